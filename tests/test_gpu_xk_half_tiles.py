"""-m gpu: conv_xk.hip runs the bottom tile row of a map with H % 16 == 8 (the 40^2 level of the 160^2 networks) on half-height tiles
(8 rows x 16 columns, 2 M tiles per wave) in the same launch as the full-height tiles.  Everything goes through
ops.conv3x3_block(..., precision='fp16x3', want_stats=True); the tolerances are those of test_conv3x3_block_ragged_tiles_fp16x3:
output < 3e-6 of the reference maximum against fp64 torch, per-tile partials within 1e-5 * max sum y^2 over the valid pixels.

The checker test at the end is a host test (no GPU): tools/check_xp_isa.py and the kernel's second template argument."""
import importlib.util
import os

import numpy as np
import pytest
import torch


def dev():
    return torch.device('cuda:0')


def _inputs(seed, B, H, W, C0, C1, Cout, norm, res):
    rs = np.random.RandomState(seed)
    Cin = C0 + C1
    t = {'x': torch.from_numpy(rs.randn(B, H, W, Cin).astype(np.float32) * 2.0 + 0.3),
         'w': torch.from_numpy((rs.randn(Cout, Cin, 3, 3) / (3.0 * Cin ** 0.5)).astype(np.float32)),
         'bias': torch.from_numpy(rs.randn(Cout).astype(np.float32)),
         'sc': torch.from_numpy((rs.rand(B, Cin) + 0.5).astype(np.float32)) if norm else None,
         'sh': torch.from_numpy((rs.randn(B, Cin) * 0.5).astype(np.float32)) if norm else None,
         'rv': torch.from_numpy((rs.randn(B, H, W, Cout) * 3.0).astype(np.float32)) if res else None}
    return t


def _run(t, C0, sl=slice(None)):
    """the block on samples `sl` of the inputs -> (y, per-tile partials [b, tile row, tile column, cout, 2]) on the host"""
    from conditional_score_diffusion_amd import ops
    d = dev()
    opt = lambda v: None if v is None else v[sl].contiguous().to(d)      # noqa: E731
    x = t['x'][sl]
    B, H, W, Cin = x.shape
    y, st = ops.conv3x3_block(x[..., :C0].contiguous().to(d), t['w'].to(d), t['bias'].to(d),
                              x1=x[..., C0:].contiguous().to(d) if Cin > C0 else None, nscale=opt(t['sc']), nshift=opt(t['sh']),
                              res=opt(t['rv']), out_scale=0.75, precision='fp16x3', want_stats=True)
    return y.cpu(), st.cpu().reshape(B, (H + 15) // 16, (W + 15) // 16, -1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize('B,H,W,C0,C1,Cout,norm,res', [
    (1, 24, 32, 64, 0, 96, False, False),     # the smallest map of the ragged domain with a partial tile row; four stages; 2 half-height items
    (3, 24, 32, 96, 0, 192, True, True),      # two cout groups; 12 half-height items: no multiple of 8
    (2, 40, 32, 96, 96, 96, True, False),     # full-width tiles only, virtual concat
    (2, 40, 40, 192, 96, 192, True, True),    # the corner tile is half-height AND half-width; 18 stages
    (1, 56, 40, 96, 0, 96, False, True),      # three full tile rows above the half row
])
def test_half_height_tiles_vs_fp64(B, H, W, C0, C1, Cout, norm, res):
    """output and per-tile GroupNorm partials (valid pixels only) against fp64 torch at the smallest shapes that can go wrong"""
    t = _inputs(H * 100 + W + B, B, H, W, C0, C1, Cout, norm, res)
    y, st = _run(t, C0)
    xd = t['x'].double()
    if norm:
        xd = torch.nn.functional.silu(xd * t['sc'].double()[:, None, None, :] + t['sh'].double()[:, None, None, :])
    ref = torch.nn.functional.conv2d(xd.permute(0, 3, 1, 2), t['w'].double(), t['bias'].double(), padding=1).permute(0, 2, 3, 1)
    if res:
        ref = ref + t['rv'].double()
    ref = ref * 0.75
    yc = y.double()
    err = (yc - ref).abs().max().item() / ref.abs().max().item()
    print('half tiles', (B, H, W, C0, C1, Cout, norm, res), 'err %.3e' % err)
    assert err < 3e-6, err
    worst = 0.0
    for i in range(st.shape[1]):
        for j in range(st.shape[2]):
            blk = yc[:, 16 * i:16 * i + 16, 16 * j:16 * j + 16, :]
            worst = max(worst, (st[:, i, j, :, 0] - blk.sum((1, 2))).abs().max().item(),
                        (st[:, i, j, :, 1] - (blk * blk).sum((1, 2))).abs().max().item() * 0.1)
    bound = 1e-5 * float((yc * yc).sum((1, 2)).max())
    print('   partials: worst %.3e, bound %.3e' % (worst, bound))
    assert worst < bound, (worst, bound)


@pytest.mark.gpu
def test_half_height_walk_tile_to_tile_is_batch_independent():
    """B = 72 of 24 x 32, 64 -> 192, GroupNorm + residual: 288 half-height items, about three per half-height workgroup - the next
    tile's first stages are requested and converted under this tile's last ones.  Every sample's output and partials must be bitwise
    what the same sample gives in a batch of 3 (one round everywhere; the small batch is pinned to fp64 above)"""
    B, H, W, C0, Cout = 72, 24, 32, 64, 192
    t = _inputs(7, B, H, W, C0, 0, Cout, True, True)
    y, st = _run(t, C0)
    for b0 in range(0, B, 3):
        y3, st3 = _run(t, C0, slice(b0, b0 + 3))
        assert torch.equal(y[b0:b0 + 3], y3), b0
        assert torch.equal(st[b0:b0 + 3], st3), b0


@pytest.mark.gpu
@pytest.mark.parametrize('res', [False, True])
@pytest.mark.parametrize('H,W,C0,Cout', [(24, 32, 96, 96), (40, 40, 96, 192)])
def test_half_height_equals_full_height_on_zero_extended_map(H, W, C0, Cout, res):
    """without the GroupNorm prologue padding zeros and data zeros coincide: the same map extended by 8 rows of zeros has full-height
    bottom tiles, whose M tiles 0 and 1 see the operands of the half-height ones - rows [0, H) of the output and the partials of the tile
    rows that lie wholly inside the image must be bitwise equal"""
    B = 2
    t = _inputs(H + W, B, H, W, C0, 0, Cout, False, res)
    y, st = _run(t, C0)
    te = dict(t)
    te['x'] = torch.cat([t['x'], torch.zeros(B, 8, W, C0)], 1)
    if res:
        te['rv'] = torch.cat([t['rv'], torch.zeros(B, 8, W, Cout)], 1)
    ye, ste = _run(te, C0)
    assert torch.equal(y, ye[:, :H])
    assert torch.equal(st[:, :H // 16], ste[:, :H // 16])


def test_isa_check_knows_the_m_tile_argument(tmp_path):
    """tools/check_xp_isa.py on synthetic listings under the four-argument kernel name: 2 NT accumulator tuples in one body pass, a read
    of an accumulator in a matrix instruction's shadow fails; a kernel of two marked walks is checked walk by walk"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('check_xp_isa', os.path.join(root, 'tools', 'check_xp_isa.py'))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    name = '_ZN3csd14conv_xk_kernelILi3ELi2ELb1ELb0EEEvPKcNS_10ConvFFArgsE'
    mf = ['\tv_mfma_f32_32x32x16_f16 a[%d:%d], a[200:203], v[6:9], a[%d:%d]' % (16 * i, 16 * i + 15, 16 * i, 16 * i + 15) for i in range(12)]
    rd = '\tds_write_b128 v1, a[0:3]'
    good = [name + ':'] + mf[:6] + ['\ts_nop 15', rd, '\ts_endpgm']
    shadow = [name + ':'] + mf[:6] + [rd, '\ts_endpgm']
    twelve = [name + ':'] + mf + ['\ts_nop 15', rd, '\ts_endpgm']                    # 4 NT tuples under an MT = 2 name
    old_name = [name.replace('Li3ELi2E', 'Li3E') + ':'] + mf + ['\ts_nop 15', rd, '\ts_endpgm']      # the three-argument name: MT = 4
    # two walks behind marks: 12 tuples, then 6 (a[96:111] of the first walk is no accumulator in the second: an LDS read may write it)
    two = ([name + ':', '\ts_cbranch_scc0 .LBB0_2', '\t; conv_xk walk MT = 4'] + mf + ['\ts_nop 15', rd, '\ts_branch .LBB0_3', '.LBB0_2:',
           '\t; conv_xk walk MT = 2'] + mf[:6] + ['\tds_read_b128 a[96:99], v3', '\ts_nop 15', rd, '\ts_endpgm'])
    two_shadow = two[:-3] + [rd, '\ts_endpgm']
    two_short = [ln for ln in two if ln != mf[11]]
    for lines, rc in ((good, 0), (shadow, 1), (twelve, 1), (old_name, 0), (two, 0), (two_shadow, 1), (two_short, 1)):
        p = tmp_path / 'k.s'
        p.write_text('\n'.join(lines) + '\n')
        assert chk.main(str(p)) == rc, lines
