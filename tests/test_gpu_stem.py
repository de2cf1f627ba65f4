"""The stem kernels -- csrc/stem.hip (conv0 read from the caller's fp32 NCHW images: the direct and the MFMA forward, the NHWC4 pack, conv0
recomputed inside its four BatchNorm / SiLU passes, the direct weight gradient) and the stem entry of csrc/conv_wgrad.hip (the weight gradient
on MFMA) -- element by element against float64 on the CPU, through the C ABI, on exactly the operands the kernel reads: where a path rounds
its operands to bf16 the host rounds them once, and the rounded tensor is both uploaded and fed to the reference.  Formulas and limits are
tests/stem_restatement.py (pinned without a GPU by tests/test_stem_restatement_cpu.py); helpers are those of tests/test_gpu_streaming.py.

Cases are chosen by LOOP REGIME, named beside each, at the smallest shape that reaches it.  M = B * H * W pixels; a tile = 16 pixels of one
image row; the MFMA forward gives a wave 16 consecutive tiles and a block 1024 pixels; the fused passes run persistent waves over chunks of
16 tiles, strided over min(ceil(M / 1024), 2048) blocks, with 4 (2 in REDUCE) tiles in flight.  FVA_STEM_MFMA is read once per process, so
the forward path is chosen by dtype and W and asserted through fva_stem_fwd_workspace.  Every test prints its n (the longest chain of fp32
additions behind one sum) and its worst err / limit (pytest -s); DESIGN section 4 carries the numbers.
"""
import pytest
import torch

import stem_restatement as sr
import streaming_measure as sm
from test_gpu_streaming import BF, FP, api, bits, case_id, dev, gpu, interior, key, nan_buf, same_bits, specials

pytestmark = pytest.mark.gpu

CO = sr.CO


def draw(B, Cin, H, W, seed, rounded):
    """image and filter bank; rounded: to bf16 once, as the MFMA paths read them (kept in fp32 storage: the entry points take fp32)"""
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, Cin, H, W, generator=g) * 0.8
    w = torch.randn(CO, Cin, 3, 3, generator=g) * 0.3
    if rounded:
        img, w = img.bfloat16().float(), w.bfloat16().float()
    return g, img, w


def report(name, regime, n, **figures):
    print(f'\n  {name} [{regime}] n = {n}: worst err / limit ' + ', '.join(f'{k} {v:.3f}' for k, v in figures.items()))


def check_y_and_stats(name, regime, got, stats, y64, yl, geometry, bf, stored_stats):
    """y per element and the [block][2][32] statistics per block row.  stored_stats: the kernel sums the values it stored (direct kernel:
    against the downloaded y by the sum rule alone); else its fp32 accumulators (MFMA kernel: against y64, with the share of ylim)."""
    M = y64.shape[0]
    owner, rows, n = geometry(M)
    assert stats.shape[0] == rows
    wy = sr.worst(got, y64, yl, bf)
    rs = sr.RowSums(rows, owner)
    if stored_stats:
        g64 = got.double()
        rs.add(0, M, (g64, g64 * g64))
    else:
        terms, extra = sr.stats_terms(y64, yl)
        rs.add(0, M, terms, extra=extra)
    ws = rs.worst(stats, n)
    figures = dict(y=wy, stats=ws)
    if bf and got.numel() >= sm.BIAS_MIN_N:
        figures['bias_ulp'] = sm.rounding_bias(got, y64)
    report(name, regime, n, **figures)
    assert wy <= 1.0 and ws <= 1.0, (regime, wy, ws)
    assert abs(figures.get('bias_ulp', 0.0)) <= sm.BIAS_MAX, (regime, figures)


# ================================================================================================ 1. fva_stem_fwd, direct kernel
#  dt  B  Cin  H   W    regime (one pixel per lane, 256 per block; bf16 stays on this kernel while W % 16 != 0)
DIRECT_CASES = [
    (FP, 1, 3, 1, 1, 'one pixel: only the centre tap is in bounds, 255 dead lanes'),
    (BF, 1, 3, 1, 1, 'one pixel, bf16'),
    (FP, 2, 3, 5, 7, 'M = 70 < one block: dead lanes add 0 to the statistics; odd H and W'),
    (BF, 2, 3, 5, 7, 'M = 70, bf16'),
    (FP, 1, 3, 16, 16, 'M = 256 exactly: one full block (fp32: bf16 at W = 16 is the MFMA kernel)'),
    (FP, 3, 1, 9, 29, 'Cin = 1, M = 783 = three blocks + 15 pixels, every block straddles images'),
    (BF, 3, 1, 9, 29, 'Cin = 1, M = 783, bf16'),
    (BF, 1, 2, 3, 100, 'Cin = 2, W = 100 (not a multiple of 16): bf16 on the direct kernel, blocks straddle rows'),
    (FP, 1, 2, 3, 100, 'Cin = 2, W = 100, fp32'),
    (BF, 2, 3, 29, 57, '105792 bf16 elements: rounding bias; 13 blocks, the last one short'),
]


@pytest.mark.parametrize('case', DIRECT_CASES, ids=case_id)
def test_stem_fwd_direct(case):
    _lib, ops = api()
    lib = _lib.load()
    dt, B, Cin, H, W, regime = case
    M, code = B * H * W, ops._code(dt)
    assert lib.fva_stem_fwd_workspace(code, B, H, W) == 0, 'this shape is served by the direct kernel'
    _, img, w = draw(B, Cin, H, W, 11 + W + Cin, rounded=False)
    y64, sabs = sr.conv64(img, w)
    nblk = lib.fva_stem_stat_blocks(code, B, H, W)
    imgd, wd = gpu(img), gpu(w)
    y, stats = nan_buf((M, CO), dt), nan_buf((nblk, 2, CO), FP)
    _lib.call('fva_stem_fwd', code, ops._p(imgd), ops._p(wd), ops._p(y), ops._p(stats), ops._p(None), 0, B, Cin, H, W, CO, ops._stream())
    y2 = nan_buf((M, CO), dt)                                      # without statistics: the same y, bit for bit
    _lib.call('fva_stem_fwd', code, ops._p(imgd), ops._p(wd), ops._p(y2), ops._p(None), ops._p(None), 0, B, Cin, H, W, CO, ops._stream())
    assert torch.equal(bits(y2.cpu()), bits(y.cpu())), regime
    check_y_and_stats(f'fva_stem_fwd direct {key(dt)}', regime, y.cpu(), stats.cpu(), y64, sr.y_limit(sr.n_direct(Cin), sabs),
                      sr.direct_stats_geometry, dt == BF, stored_stats=True)


# ================================================================================================ 2. fva_stem_pack, fva_stem_fwd MFMA kernel
#  B  Cin  H   W    regime (tiles per row = W / 16; a wave walks 16 consecutive tiles, a block 64)
MFMA_CASES = [
    (1, 3, 1, 16, 'one tile: waves 1-3 of the only block idle'),
    (3, 3, 2, 16, 'one tile per row: every tile wraps a row, every second one an image; M / 16 = 6'),
    (3, 3, 5, 48, 'three tiles per row: a wave\'s 16 tiles cross rows and an image unevenly; M = 720 < one block; M / 16 = 45 (odd, = 1 mod 4)'),
    (1, 1, 64, 16, 'Cin = 1, M = 1024: exactly one block, every wave full'),
    (2, 3, 33, 32, 'M = 2112: two blocks and a short third whose last waves have nothing to do; M / 16 = 132'),
]
PACK_CASES = MFMA_CASES + [
    (2, 2, 3, 32, 'Cin = 2: channels 2 and 3 zero'),
    (1, 1, 4100, 4096, '16809996 halo pixels > 65536 blocks x 256 threads: the grid-stride loop of the pack kernel takes a second trip'),
]
FWD_MFMA_CASES = MFMA_CASES + [(1, 3, 16, 208, '106496 bf16 elements: rounding bias; 13 tiles per row, 4 blocks, the last one a quarter full')]


@pytest.mark.parametrize('case', PACK_CASES, ids=case_id)
def test_stem_pack(case):
    """bit for bit: interior = torch's own cast of the image (specials planted), border and channels >= Cin +0, every pixel overwritten in a
    buffer pre-filled with 0xFF bytes, the 64 slack bytes behind it untouched"""
    _lib, ops = api()
    lib = _lib.load()
    B, Cin, H, W, regime = case
    g = torch.Generator().manual_seed(W + H)
    img = specials(torch.randn(B, Cin, H, W, generator=g))
    need = lib.fva_stem_fwd_workspace(_lib.BF16, B, H, W)
    assert need == B * (H + 2) * (W + 2) * 8 + 64
    imgd = gpu(img)
    buf = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev())
    _lib.call('fva_stem_pack', ops._p(imgd), ops._p(buf), need, B, Cin, H, W, ops._stream())
    got = buf.cpu().view(BF)
    want = sr.pack_host(img.bfloat16(), slack=-1)
    assert torch.equal(bits(got[-32:]), bits(want[-32:])), f'{regime}: the slack bytes are untouched'
    same_bits(got[:-32].view(B, H + 2, W + 2, 4), want[:-32].view(B, H + 2, W + 2, 4), f'fva_stem_pack [{regime}]')
    print(f'\n  fva_stem_pack [{regime}]: bit-exact, border / unused channels +0, slack untouched')


@pytest.mark.parametrize('case', FWD_MFMA_CASES, ids=case_id)
def test_stem_fwd_mfma(case):
    _lib, ops = api()
    lib = _lib.load()
    B, Cin, H, W, regime = case
    M = B * H * W
    wsb = lib.fva_stem_fwd_workspace(_lib.BF16, B, H, W)
    assert wsb > 0, 'this shape is served by the MFMA kernel (FVA_STEM_MFMA must not be 0)'
    _, img, w = draw(B, Cin, H, W, 23 + W + H, rounded=True)
    y64, sabs = sr.conv64(img, w)
    nblk = lib.fva_stem_stat_blocks(_lib.BF16, B, H, W)
    imgd, wd = gpu(img), gpu(w)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=dev())
    y, stats = nan_buf((M, CO), BF), nan_buf((nblk, 2, CO), FP)
    _lib.call('fva_stem_fwd', _lib.BF16, ops._p(imgd), ops._p(wd), ops._p(y), ops._p(stats), ops._p(ws), wsb, B, Cin, H, W, CO, ops._stream())
    y2 = nan_buf((M, CO), BF)                                      # without statistics: the same y, bit for bit
    _lib.call('fva_stem_fwd', _lib.BF16, ops._p(imgd), ops._p(wd), ops._p(y2), ops._p(None), ops._p(ws), wsb, B, Cin, H, W, CO, ops._stream())
    assert torch.equal(bits(y2.cpu()), bits(y.cpu())), regime
    check_y_and_stats('fva_stem_fwd mfma bf16', regime, y.cpu(), stats.cpu(), y64, sr.y_limit(sr.N_MFMA, sabs), sr.mfma_stats_geometry, True,
                      stored_stats=False)


# ================================================================================================ 3. fva_stem_fused, modes 0..3
#  B  Cin  H    W     regime (chunks = ceil(M / 256); prefetch groups of 4 tiles, 2 in REDUCE: the ok[] tail cuts a group where M / 16 is
#                     not a multiple of the depth)
FUSED_CASES = [
    (1, 3, 1, 16, 'M / 16 = 1: one tile, the first prefetch group holds three (REDUCE: one) dead slots'),
    (3, 3, 2, 16, 'M / 16 = 6 = 2 mod 4: row wrap after every tile, image wrap after every second; the second group of four is half dead, REDUCE\'s groups of two are all full'),
    (3, 3, 5, 48, 'M / 16 = 45 = 1 mod 4, odd: chunks cross rows and images unevenly, the last chunk ends inside a group in both depths; 3 chunks in one block'),
    (1, 1, 64, 16, 'Cin = 1, M / 16 = 64: four full chunks, one per wave, no tail'),
    (2, 3, 33, 32, 'M / 16 = 132 = 0 mod 4: 9 chunks over 3 blocks, the last chunk 4 tiles long (one group; REDUCE two)'),
    (2, 2, 3, 32, 'Cin = 2, M / 16 = 12: one short chunk that wraps rows and an image'),
    (2, 3, 1032, 1024, 'M = 2113536 > 2048 * 1024: 8256 chunks over 2048 blocks, blocks 0..15 take a second chunk (the persistent loop); rounding bias'),
]


@pytest.mark.parametrize('case', FUSED_CASES, ids=case_id)
def test_stem_fused(case):
    """all four modes on one set of operands: the packed image (made on the host), bf16(weights), bf16 dz and per-channel tables made from
    the float64 statistics of y64.  The reference is evaluated band by band (bounded host memory), every element compared."""
    _lib, ops = api()
    lib = _lib.load()
    B, Cin, H, W, regime = case
    M = B * H * W
    blocks = lib.fva_stem_fused_blocks(B, H, W)
    assert blocks == min(sr.cdiv(M, 1024), 2048)
    owner, rounds, n = sr.fused_geometry(M, blocks)
    g, img, w = draw(B, Cin, H, W, 37 + W + H, rounded=True)
    dz = torch.randn(M, CO, generator=g).bfloat16()
    gamma, beta = sr.draw_gamma_beta(g)
    # pass 1 on the host: the statistics of y64, and realistic backward sums (those of the first band, per pixel)
    s1, s2 = torch.zeros(CO, dtype=sr.F64), torch.zeros(CO, dtype=sr.F64)
    for b, r0, r1, m0, m1 in sr.bands(B, H, W):
        y64, _ = sr.conv_rows(img, w, b, r0, r1)
        s1 += y64.sum(0)
        s2 += (y64 * y64).sum(0)
    zero = torch.zeros(CO, dtype=sr.F64)
    t0 = sr.Tables(s1, s2, M, gamma, beta, zero, zero)
    b, r0, r1, m0, m1 = next(sr.bands(B, H, W))
    du, dux = sm.bwd_terms(dz[m0:m1], sr.conv_rows(img, w, b, r0, r1)[0], t0.scale, t0.shift, t0.mean, t0.rstd, sr.F64)
    t = sr.Tables(s1, s2, M, gamma, beta, du.mean(0), dux.mean(0))
    # the four launches
    img4 = gpu(sr.pack_host(img.bfloat16()))
    wd, dzd = gpu(w), gpu(dz)
    sc, sh, mu, rs, cf = (gpu(x) for x in (t.scale, t.shift, t.mean, t.rstd, t.coef()))
    part_s, part_r = nan_buf((blocks, 2, CO), FP), nan_buf((blocks, 2, CO), FP)
    out_a, out_d = nan_buf((B, H + 2, W + 2, CO), BF), nan_buf((B, H + 2, W + 2, CO), BF)

    def launch(mode, out, part):
        _lib.call('fva_stem_fused', mode, ops._p(img4), ops._p(wd), ops._p(dzd), ops._p(sc), ops._p(sh), ops._p(mu), ops._p(rs), ops._p(cf),
                  ops._p(out), ops._p(part), B, Cin, H, W, ops._stream())
    launch(0, None, part_s)
    launch(1, out_a, None)
    launch(2, None, part_r)
    launch(3, out_d, None)
    torch.cuda.synchronize()
    z = interior(out_a.cpu(), 1, regime + ' (APPLY)').reshape(M, CO)
    dY = interior(out_d.cpu(), 1, regime + ' (DGRAD)').reshape(M, CO)
    # pass 2 on the host: every element, band by band
    st, rd = sr.RowSums(blocks, owner), sr.RowSums(blocks, owner)
    wa = wd_ = 0.0
    bias_a = bias_d = 0.0
    ulo, uhi = float('inf'), float('-inf')
    for b, r0, r1, m0, m1 in sr.bands(B, H, W):
        y64, sabs = sr.conv_rows(img, w, b, r0, r1)
        yl = sr.y_limit(sr.N_MFMA, sabs)
        u = y64 * t.scale.double() + t.shift.double()
        ulo, uhi = min(ulo, u.min().item()), max(uhi, u.max().item())
        terms, extra = sr.stats_terms(y64, yl)
        st.add(m0, m1, terms, extra=extra)
        z64, zlim = sr.apply_ref(y64, yl, t)
        wa = max(wa, sr.worst(z[m0:m1], z64, zlim, True))
        bias_a += sm.rounding_bias(z[m0:m1], z64) * (m1 - m0) / M
        t64, e32, extra = sr.reduce_terms(dz[m0:m1], y64, yl, t)
        rd.add(m0, m1, t64, e32, extra)
        r64, rlim = sr.dgrad_ref(dz[m0:m1], y64, yl, t)
        wd_ = max(wd_, sr.worst(dY[m0:m1], r64, rlim, True))
        bias_d += sm.rounding_bias(dY[m0:m1], r64) * (m1 - m0) / M
    ws, wr = st.worst(part_s.cpu(), n), rd.worst(part_r.cpu(), n)
    figures = dict(STATS=ws, APPLY=wa, REDUCE=wr, DGRAD=wd_)
    big = M * CO >= sm.BIAS_MIN_N
    if big:
        figures.update(APPLY_bias_ulp=bias_a, DGRAD_bias_ulp=bias_d)
    report('fva_stem_fused', regime + f'; {rounds} round(s), u in [{ulo:.1f}, {uhi:.1f}]', n, **figures)
    if M * CO >= 1000000:
        assert ulo < -12 and uhi > 12, 'u reaches both tails of the sigmoid'
    assert max(ws, wa, wr, wd_) <= 1.0, (regime, figures)
    if big:
        assert abs(bias_a) <= sm.BIAS_MAX and abs(bias_d) <= sm.BIAS_MAX, (regime, figures)


# ================================================================================================ 4. fva_stem_wgrad (direct kernel)
#  dt  B  Cin  H    W   accumulate  regime (tiles of 128 pixels over min(tiles, 1024) blocks)
WGRAD_CASES = [
    (FP, 1, 3, 3, 7, 0, 'M = 21 < one 128-pixel tile'),
    (BF, 1, 3, 3, 7, 1, 'M = 21, bf16 dy, accumulate onto a pre-filled dw'),
    (FP, 2, 1, 9, 29, 1, 'Cin = 1 (lanes with j4 * 4 >= 9 idle), M = 522 = 4 tiles + 10 pixels, tiles straddle images; accumulate'),
    (BF, 2, 1, 9, 29, 0, 'Cin = 1, M = 522, bf16 dy'),
    (BF, 1, 2, 3, 100, 0, 'Cin = 2, M = 300'),
    (BF, 2, 3, 260, 256, 0, '1040 tiles > 1024 blocks: blocks 0..15 take a second tile (the grid-stride loop); the reduce adds 4 partials per lane'),
    (FP, 2, 3, 260, 256, 0, '1040 tiles > 1024 blocks, fp32 dy'),
]


@pytest.mark.parametrize('case', WGRAD_CASES, ids=case_id)
def test_stem_wgrad(case):
    _lib, ops = api()
    lib = _lib.load()
    dt, B, Cin, H, W, accumulate, regime = case
    M = B * H * W
    g, img, _ = draw(B, Cin, H, W, 53 + W + Cin, rounded=False)
    dy = torch.randn(B, H, W, CO, generator=g).to(dt)
    pre = torch.randn(CO, Cin, 3, 3, generator=g)
    ref, sabs = sr.wgrad64(img, dy)
    n, ntiles, grid = sr.wgrad_chain(M)
    wsb = lib.fva_stem_wgrad_workspace(B, Cin, H, W, CO)
    imgd, dyd = gpu(img), gpu(dy)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev())
    dw = gpu(pre) if accumulate else nan_buf((CO, Cin, 3, 3), FP)
    _lib.call('fva_stem_wgrad', ops._code(dt), ops._p(imgd), ops._p(dyd), ops._p(dw), accumulate, ops._p(ws), wsb, B, Cin, H, W, CO, ops._stream())
    wst = sr.wgrad_worst(dw.cpu(), ref, sabs, n, pre if accumulate else None)
    report(f'fva_stem_wgrad {key(dt)} accumulate={accumulate}', regime + f'; {ntiles} tiles on {grid} blocks', n, dw=wst)
    assert wst <= 1.0, (regime, wst)


# ================================================================================================ 5. fva_stem_wgrad_mfma
#  B  Cin  H   W    regime (split-K blocks of mchunk = 64 * ceil(M / 512 / 64) pixels, k-steps of 64)
WGRAD_MFMA_CASES = [
    (1, 3, 1, 16, 'M = 16 < one 64-row k-step: 48 rows of the only step read the zero corner of dy'),
    (3, 3, 5, 48, 'M = 720: 12 splits of 64, the last one 16 rows long'),
    (2, 2, 3, 32, 'Cin = 2: the packed image\'s channel 2 is zero'),
    (1, 3, 65, 512, 'M = 33280 > 32768: mchunk becomes 128 (two k-steps per block), 260 splits'),
]


@pytest.mark.parametrize('case', WGRAD_MFMA_CASES, ids=case_id)
def test_stem_wgrad_mfma(case):
    """raw[32][4][4][3] = [co][kw][ci][kh] in a NaN-filled buffer; its kw = 3 column and its channels >= Cin are junk by contract.  dy is a
    halo buffer with a +0 border, as the fused DGRAD pass leaves it."""
    _lib, ops = api()
    lib = _lib.load()
    B, Cin, H, W, regime = case
    M = B * H * W
    g, img, _ = draw(B, Cin, H, W, 71 + W + H, rounded=True)
    dy = torch.randn(B, H, W, CO, generator=g).bfloat16()
    dyh = torch.zeros(B, H + 2, W + 2, CO, dtype=BF)
    dyh[:, 1:-1, 1:-1] = dy
    ref, sabs = sr.wgrad64(img, dy)
    n, mchunk, ksplit = sr.wgrad_mfma_chain(M)
    img4, dyd = gpu(sr.pack_host(img.bfloat16())), gpu(dyh)
    wb = lib.fva_stem_wgrad_mfma_workspace()
    assert wb >= ksplit * 3 * 32 * 16 * 4
    ws = torch.empty(wb, dtype=torch.uint8, device=dev())
    raw = nan_buf((CO, 4, 4, 3), FP)
    _lib.call('fva_stem_wgrad_mfma', ops._p(img4), ops._p(dyd), ops._p(raw), ops._p(ws), wb, B, H, W, ops._stream())
    got = raw.cpu()[:, :3, :Cin, :].permute(0, 2, 3, 1)            # [co][ci][kh][kw]
    wst = sr.wgrad_worst(got, ref, sabs, n)
    report('fva_stem_wgrad_mfma', regime + f'; mchunk {mchunk}, {ksplit} splits', n, dw=wst)
    assert wst <= 1.0, (regime, wst)
