"""The measure of tests/test_gpu_stem.py (tests/stem_restatement.py), pinned without a GPU on one small shape with bf16 operands (the MFMA
paths): an honest device evaluation -- one chain of fp32 fmas per output, every later formula in plain fp32 torch ops, stored ONCE -- must pass
every limit, and the wrong kernels the GPU tests are there to catch must be rejected by the same limits: a tap dropped on one image row, two
swapped channels, a truncating store, operands that were not rounded to bf16, an output written one halo column off, a statistics row that sums
a neighbouring block's pixels, a weight gradient that leaves out one tile."""
import pytest
import torch

import stem_restatement as sr
import streaming_measure as sm

B, CIN, H, W = 3, 3, 40, 48           # M = 5760 pixels, 184320 outputs (enough for the rounding bias), 23 chunks of 256 pixels
M = B * H * W
BLOCKS = 2                            # an invented fused grid of 2 blocks: 8 wave slots, so a wave visits up to 3 chunks


def truncate_to_bf16(x32):
    return (x32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


@pytest.fixture(scope='module')
def data():
    g = torch.Generator().manual_seed(20240611)
    img = torch.randn(B, CIN, H, W, generator=g) * 0.8
    w = torch.randn(sr.CO, CIN, 3, 3, generator=g) * 0.3
    imgb, wb = img.bfloat16(), w.bfloat16().float()
    dz = torch.randn(M, sr.CO, generator=g).bfloat16()
    y64, sabs = sr.conv64(imgb, wb)
    yl = sr.y_limit(sr.N_MFMA, sabs)
    gamma, beta = sr.draw_gamma_beta(g)
    t0 = sr.Tables(y64.sum(0), (y64 * y64).sum(0), M, gamma, beta, torch.zeros(sr.CO, dtype=torch.float64), torch.zeros(sr.CO, dtype=torch.float64))
    du, dux = sm.bwd_terms(dz, y64, t0.scale, t0.shift, t0.mean, t0.rstd, torch.float64)
    t = sr.Tables(y64.sum(0), (y64 * y64).sum(0), M, gamma, beta, du.mean(0), dux.mean(0))
    y32 = sr.conv_fma32(imgb.float(), wb)
    return dict(img=img, w=w, imgb=imgb, wb=wb, dz=dz, y64=y64, yl=yl, t=t, y32=y32)


def device_apply(y32, t):
    return sm.silu_apply(y32, t.scale, t.shift, None, torch.float32)[0]


def device_dgrad(dz, y32, t):
    return sm.bwd_apply(dz, y32, t.scale, t.shift, t.mean, t.rstd, t.a, t.cb, t.cc, torch.float32)[0]


def device_rows(terms, owner, rows):
    """[rows][2][32] fp32 partial tables the way a device adds them: fp32 values, added in fp32 in pixel order"""
    out = torch.zeros(rows, 2, sr.CO)
    for k in range(2):
        out[:, k].index_add_(0, owner, terms[k].float())
    return out


def test_the_small_shape_is_inside_the_regimes(data):
    u = data['y64'] * data['t'].scale.double() + data['t'].shift.double()
    assert u.min() < -6 and u.max() > 6
    assert data['y64'].numel() >= sm.BIAS_MIN_N


def test_honest_fma_chain_passes_the_y_limit(data):
    y64, yl, y32 = data['y64'], data['yl'], data['y32']
    w32 = sr.worst(y32, y64, yl, False)
    yb = y32.bfloat16()
    wbf, bias = sr.worst(yb, y64, yl, True), sm.rounding_bias(yb, y64)
    print(f'honest fma chain: fp32 {w32:.3f}, stored as bf16 {wbf:.3f} of the limit, bias {bias:+.4f} ulp')
    assert w32 <= 1.0 and wbf <= 1.0 and abs(bias) <= sm.BIAS_MAX
    # the direct kernel on unrounded fp32 operands, n = 9 * Cin
    yd64, sabs = sr.conv64(data['img'], data['w'])
    assert sr.worst(sr.conv_fma32(data['img'], data['w']), yd64, sr.y_limit(sr.n_direct(CIN), sabs), False) <= 1.0


def test_honest_fused_passes_are_accepted(data):
    y64, yl, y32, t, dz = (data[k] for k in ('y64', 'yl', 'y32', 't', 'dz'))
    z64, zlim = sr.apply_ref(y64, yl, t)
    z = device_apply(y32, t)
    wa32, wa16 = sr.worst(z, z64, zlim, False), sr.worst(z.bfloat16(), z64, zlim, True)
    r64, rlim = sr.dgrad_ref(dz, y64, yl, t)
    d = device_dgrad(dz, y32, t)
    wd32, wd16 = sr.worst(d, r64, rlim, False), sr.worst(d.bfloat16(), r64, rlim, True)
    print(f'APPLY fp32 {wa32:.3f} bf16 {wa16:.3f}; DGRAD fp32 {wd32:.3f} bf16 {wd16:.3f} of the limit')
    assert max(wa32, wa16, wd32, wd16) <= 1.0
    assert abs(sm.rounding_bias(z.bfloat16(), z64)) <= sm.BIAS_MAX and abs(sm.rounding_bias(d.bfloat16(), r64)) <= sm.BIAS_MAX
    # the partial tables of an invented 2-block grid (chunks strided over 8 wave slots)
    owner, rounds, n = sr.fused_geometry(M, BLOCKS)
    assert rounds == 3 and n == 54
    st = sr.RowSums(BLOCKS, owner)
    terms, extra = sr.stats_terms(y64, yl)
    st.add(0, M, terms, extra=extra)
    ws = st.worst(device_rows((y32, y32 * y32), owner, BLOCKS), n)
    rd = sr.RowSums(BLOCKS, owner)
    t64, e32, extra = sr.reduce_terms(dz, y64, yl, t)
    rd.add(0, M, t64, e32, extra)
    wr = rd.worst(device_rows(sm.bwd_terms(dz, y32, t.scale, t.shift, t.mean, t.rstd, torch.float32), owner, BLOCKS), n)
    print(f'STATS {ws:.3f}, REDUCE {wr:.3f} of the limit')
    assert ws <= 1.0 and wr <= 1.0


def test_dropped_tap_on_one_image_row_is_rejected(data):
    """a kernel that takes row 1 of image 1 for the top border: channel 1's tap (kh 0, kw 1) is missing there"""
    bad = data['y32'].clone().view(B, H, W, sr.CO)
    bad[1, 1] -= data['imgb'][1, 1, 0, :, None].float() * data['wb'][:, 1, 0, 1]
    w = sr.worst(bad.view(M, sr.CO), data['y64'], data['yl'], False)
    wb = sr.worst(bad.view(M, sr.CO).bfloat16(), data['y64'], data['yl'], True)
    print(f'dropped tap: {w:.3g} (fp32), {wb:.3g} (bf16) x the limit')
    assert w > 100 and wb > 1.0
    # and through APPLY, where y is never seen
    z64, zlim = sr.apply_ref(data['y64'], data['yl'], data['t'])
    assert sr.worst(device_apply(bad.view(M, sr.CO), data['t']).bfloat16(), z64, zlim, True) > 1.0


def test_two_swapped_channels_are_rejected(data):
    bad = data['y32'].clone()
    bad[:, [5, 6]] = data['y32'][:, [6, 5]]
    assert sr.worst(bad.bfloat16(), data['y64'], data['yl'], True) > 100
    z64, zlim = sr.apply_ref(data['y64'], data['yl'], data['t'])
    assert sr.worst(device_apply(bad, data['t']).bfloat16(), z64, zlim, True) > 100


def test_truncating_store_is_rejected(data):
    got = truncate_to_bf16(data['y32'])
    w, b = sr.worst(got, data['y64'], data['yl'], True), sm.rounding_bias(got, data['y64'])
    print(f'truncating store of y: {w:.3f} x the limit, bias {b:+.4f} ulp')
    assert w > 1.0 and b < -0.4
    z64, zlim = sr.apply_ref(data['y64'], data['yl'], data['t'])
    got = truncate_to_bf16(device_apply(data['y32'], data['t']))
    assert sr.worst(got, z64, zlim, True) > 1.0 and sm.rounding_bias(got, z64) < -0.4


def test_unrounded_operands_on_the_mfma_path_are_rejected(data):
    got = sr.conv_fma32(data['img'], data['w'])
    w = sr.worst(got.bfloat16(), data['y64'], data['yl'], True)
    print(f'operands not rounded to bf16: {w:.3g} x the limit')
    assert w > 1.0 and sr.worst(got, data['y64'], data['yl'], False) > 100


def test_output_one_halo_column_off_is_rejected(data):
    z64, zlim = sr.apply_ref(data['y64'], data['yl'], data['t'])
    z = device_apply(data['y32'], data['t']).bfloat16().view(B, H, W, sr.CO)
    buf = torch.zeros(B, H + 2, W + 2, sr.CO, dtype=torch.bfloat16)
    buf[:, 1:-1, 2:] = z                                            # one column to the right: the last one lands on the border
    assert buf[:, :, -1].abs().sum() > 0, 'the border check of the GPU test sees it'
    assert sr.worst(buf[:, 1:-1, 1:-1].reshape(M, sr.CO), z64, zlim, True) > 100


def test_statistics_row_of_the_neighbouring_block_is_rejected(data):
    y64, yl, y32 = data['y64'], data['yl'], data['y32']
    owner, nrows, n = sr.mfma_stats_geometry(M)
    assert nrows == 6 and n == 22
    st = sr.RowSums(nrows, owner)
    terms, extra = sr.stats_terms(y64, yl)
    st.add(0, M, terms, extra=extra)
    good = device_rows((y32, y32 * y32), owner, nrows)
    assert st.worst(good, n) <= 1.0
    assert st.worst(torch.roll(good, 1, 0), n) > 100
    # the totals alone would not see it
    assert torch.allclose(torch.roll(good, 1, 0).sum(0), good.sum(0))
    # a NaN in a row is not a pass
    good[2, 1, 7] = float('nan')
    assert st.worst(good, n) == float('inf')


def test_weight_gradient_limit(data):
    dy = data['dz'].view(B, H, W, sr.CO)
    ref, sabs = sr.wgrad64(data['imgb'], dy)
    cols = torch.nn.functional.unfold(data['imgb'].float(), 3, padding=1).permute(0, 2, 1).reshape(M, CIN * 9)
    d = dy.reshape(M, sr.CO).float()
    acc = torch.zeros(sr.CO, CIN * 9)
    for m in range(M):                                              # the longest chain there can be: every pixel in one fp32 chain
        acc = acc + d[m, :, None] * cols[m]
    w = sr.wgrad_worst(acc.view(sr.CO, CIN, 3, 3), ref, sabs, M)
    print(f'weight gradient, one chain of {M}: {w:.3f} of the limit')
    assert w <= 1.0
    n, ntiles, grid = sr.wgrad_chain(M)
    assert (n, ntiles, grid) == (32 + 2 + 1 + 8, 45, 45)
    assert sr.wgrad_chain(2 * 260 * 256) == (64 + 2 + 4 + 8, 1040, 1024)
    assert sr.wgrad_mfma_chain(65 * 512) == (128 + 65 + 2, 128, 260) and sr.wgrad_mfma_chain(16)[1:] == (64, 1)
    tree = (d.double().t() @ cols.double()).float().view(sr.CO, CIN, 3, 3)     # a well-ordered sum passes the device's n
    assert sr.wgrad_worst(tree, ref, sabs, n) <= 1.0
    less = ((d[128:].double().t() @ cols[128:].double())).float().view(sr.CO, CIN, 3, 3)       # the first tile left out
    assert sr.wgrad_worst(less, ref, sabs, n) > 100
    pre = torch.randn(sr.CO, CIN, 3, 3, generator=torch.Generator().manual_seed(3))
    assert sr.wgrad_worst(pre + tree, ref, sabs, n, pre) <= 1.0
    assert sr.wgrad_worst(tree, ref, sabs, n, pre) > 100             # accumulate ignored


def test_pack_host_layout(data):
    buf = sr.pack_host(data['imgb'][:, :2], slack=-1)
    assert buf.numel() == B * (H + 2) * (W + 2) * 4 + 32
    p = buf[:-32].view(B, H + 2, W + 2, 4)
    assert torch.equal(p[:, 1:-1, 1:-1, :2], data['imgb'][:, :2].permute(0, 2, 3, 1))
    assert not p[..., 2:].view(torch.int16).any() and not p[:, 0].view(torch.int16).any() and not p[:, :, -1].view(torch.int16).any()
    assert (buf[-32:].view(torch.int16) == -1).all()
