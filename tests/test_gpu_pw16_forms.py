"""-m gpu: every form of the pointwise fp16 kernel (conv_pw16.hip: pw16_kernel's FULL / RES / NORM instantiations, 64- and 128-pixel
tiles), in 'fp16x3' and 'fp16'.

Op level: ops.conv2d against an fp64 product, at test_gpu_ops.test_conv2d_fp16_mfma's bound.
Network level: tiny planned networks against the same network in csd_precision = 'fp32' (which runs no pw16 layer), at
test_gpu_network.test_fp16_mfma_modes_vs_golden's network bound.  nf = 32, ch_mult (1, 2), attention at both levels; between them the
networks run
  * the two-source NIN shortcut (64 + 32 -> 32 and 64 + 64 -> 64 channels, no residual, no GroupNorm),
  * q / k / v with the GroupNorm scale / shift rows in the loader,
  * NIN_3 with its residual,
  * the tap-partial head (32 -> 27 partial channels: 2 of 6 cout tiles) with GroupNorm + SiLU in the loader,
at batch sizes on both sides of the 768-tile threshold between the 64- and the 128-pixel-tile kernel:
  64^2 at B = 24 is 98 304 pixels = exactly 768 tiles of 128; 36^2 at B = 76 is 98 496 pixels with 1296 pixels per sample, so tiles
  straddle samples and the per-pixel GroupNorm row matters; B = 2 of both runs the 64-pixel tiles."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
import score_oracle as so  # noqa: E402

PRECISIONS = [('fp16x3', 2e-6, 1e-4), ('fp16', 2e-3, 2e-2)]       # precision, test_conv2d_fp16_mfma's tol, test_fp16_mfma_modes_vs_golden's tol_net


def dev():
    return torch.device('cuda:0')


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rnd(*s, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*s, generator=g) * scale


# ---- op level ------------------------------------------------------------------------------------------------------------------
OP_CASES = [
    # B, Cin, Cout, H
    (3, 192, 96, 184),     # 101 568 pixels: the 128-pixel-tile kernel (794 tiles), ragged last tile, all 96 couts (FULL)
    (2, 40, 200, 7),       # Cin padded to 32, three cout groups (the last: one tile), ragged pixel tail
    (1, 96, 28, 16),       # a narrow group: 2 of 6 tiles, the second one ragged (12 couts)
    (1, 96, 200, 16),      # two full groups and a last group of 1 tile
]


@functools.lru_cache(maxsize=None)
def op_case(B, Cin, Cout, H):
    """inputs and the fp64 reference of one case, computed once for both precisions"""
    x = rnd(B, Cin, H, H, seed=1)
    w = rnd(Cout, Cin, 1, 1, seed=2, scale=(1.0 / Cin) ** 0.5)
    b = rnd(Cout, seed=3, scale=0.1)
    ref = torch.einsum('oc,bchw->bohw', w[:, :, 0, 0].double(), x.double()) + b.double()[None, :, None, None]
    return x, w, b, ref


@pytest.mark.parametrize('B,Cin,Cout,H', OP_CASES)
@pytest.mark.parametrize('precision,tol,_tol_net', PRECISIONS)
def test_pointwise_conv_forms_vs_fp64(B, Cin, Cout, H, precision, tol, _tol_net):
    from conditional_score_diffusion_amd import ops
    x, w, b, ref = op_case(B, Cin, Cout, H)
    out = ops.conv2d(x.to(dev()), w.to(dev()), b.to(dev()), precision=precision)
    assert out.shape == ref.shape
    err = rel(out, ref)
    print('pw16 %s B=%d %d->%d %dx%d: %.3e' % (precision, B, Cin, Cout, H, H, err))
    assert err < tol * max(1, (Cin * 9) ** 0.5 / 8)


# ---- network level -------------------------------------------------------------------------------------------------------------
NETS = {64: 24, 36: 76}          # image size -> the batch that puts the full-resolution level on the 128-pixel tiles


@functools.lru_cache(maxsize=None)
def net_model(S, precision):
    from conditional_score_diffusion_amd.models import utils as mutils
    cfg = cases.make_config(name='ddpm_paired_SR3', nf=32, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(S, S // 2), image_size=S)
    cfg.model.csd_precision = precision
    nc = so.NetCfg.from_config(cfg)
    p = so.synth_params(so.ddpm_param_shapes(nc), 0)
    model = mutils.create_model(cfg)
    missing = model.load_state_dict(p)
    assert not missing.missing_keys and not missing.unexpected_keys
    return model.to(dev()).eval()


@functools.lru_cache(maxsize=None)
def net_inputs(S):
    B = NETS[S]
    rs = np.random.RandomState(S)
    x = torch.from_numpy(rs.standard_normal((B, 3, S, S)).astype(np.float32) * 5).to(dev())
    y = torch.from_numpy(rs.uniform(0, 1, (B, 3, S, S)).astype(np.float32)).to(dev())
    lab = torch.from_numpy(rs.uniform(0, 999, (B,)).astype(np.float32)).to(dev())
    return x, y, lab


@functools.lru_cache(maxsize=None)
def net_out(S, precision, B):
    """the network on the first B samples of net_inputs(S); the fp32 outputs are the references, computed once"""
    x, y, lab = net_inputs(S)
    with torch.no_grad():
        out = net_model(S, precision)({'x': x[:B].contiguous(), 'y': y[:B].contiguous()}, lab[:B].contiguous())
    return out.cpu()


@pytest.mark.parametrize('S', sorted(NETS))
@pytest.mark.parametrize('big', [False, True], ids=['tiles64', 'tiles128'])
@pytest.mark.parametrize('precision,_tol,tol_net', PRECISIONS)
def test_network_pointwise_forms_vs_fp32_network(S, big, precision, _tol, tol_net):
    B = NETS[S] if big else 2
    out, ref = net_out(S, precision, B), net_out(S, 'fp32', B)
    assert torch.isfinite(out).all()
    err = rel(out, ref)
    print('pw16 forms %s %dx%d B=%d: %.3e' % (precision, S, S, B, err))
    assert err < tol_net


@pytest.mark.parametrize('S', sorted(NETS))
@pytest.mark.parametrize('precision,_tol,_tol_net', PRECISIONS)
def test_large_batch_sample_equals_the_single_sample_run(S, precision, _tol, _tol_net):
    """sample 0 of the large batch (128-pixel tiles, tiles that straddle samples at 36^2) against the B = 1 run (64-pixel tiles): bit for bit"""
    big, one = net_out(S, precision, NETS[S]), net_out(S, precision, 1)
    assert torch.equal(big[:1], one), float((big[:1] - one).abs().max())
