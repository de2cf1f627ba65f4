"""The streaming kernels around the convolutions -- csrc/bn_act.hip (BatchNorm + SiLU + residual forward and backward, FPN
upsample / concat, the two layout converters) and csrc/head.hip (head-gradient repack, bias gradient) -- element by element against
float64 on the CPU, computed from exactly the operands the kernel reads (bf16 inputs are made on the host, rounded once, and that
rounded tensor is both uploaded and fed to the reference).  The measure is tests/streaming_measure.py (pinned without a GPU by
tests/test_streaming_measure_cpu.py): fp32 outputs within 4 x (32 x where a sigmoid is evaluated: derived in that module) the error of a
plain fp32 torch evaluation + 2^-24 of the largest term; bf16 outputs within HALF A BF16 ULP of the float64 result on top of that, and unbiased; sums by the (n + 2) * 2^-24 * sum|term|
rule; copies and casts bit for bit; halo borders +0 bit for bit in outputs allocated full of NaN.

Cases are chosen by LOOP REGIME, named beside each: cpp = 16-byte chunks per pixel = C / 8 (bf16) or C / 4 (fp32); row_chunks =
(W + 2 * pad) * cpp; the apply kernels run 256 threads with 2 chunks in flight per thread and step.  Every test prints its worst
err / limit (pytest -s); DESIGN section 4 carries the numbers.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import streaming_measure as sm

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float32
TOL = {'f32': 1e-4, 'bf16': 1e-2}          # tests/test_gpu_kernels.py: the implicit-GEMM tolerance (fva_head_fwd is that kernel)
NAN = float('nan')


def dev():
    return torch.device('cuda:0')


def gpu(t):
    return None if t is None else t.to(dev())


def api():
    from fastvision_amd import _lib, ops
    return _lib, ops


def nan_buf(shape, dt):
    return torch.full(shape, NAN, dtype=dt, device=dev())


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def interior(buf, pad, what=''):
    """A downloaded halo output: nothing is NaN, the border is +0 bit for bit; returns the interior."""
    assert not torch.isnan(buf).any(), f'{what}: NaN left in the output'
    if pad == 0:
        return buf
    Hp, Wp = buf.shape[1], buf.shape[2]
    border = torch.ones(Hp, Wp, dtype=torch.bool)
    border[pad:Hp - pad, pad:Wp - pad] = False
    assert not bits(buf)[:, border].any(), f'{what}: the border is not +0'
    return buf[:, pad:Hp - pad, pad:Wp - pad]


def in_halo(t, pad):
    """An INPUT halo buffer around the dense NHWC tensor t whose border is NaN: a kernel that reads one pixel off shows it."""
    if pad == 0:
        return t.contiguous()
    B, H, W, Cc = t.shape
    buf = torch.full((B, H + 2 * pad, W + 2 * pad, Cc), NAN, dtype=t.dtype)
    buf[:, pad:pad + H, pad:pad + W] = t
    return buf


def key(dt):
    return 'bf16' if dt == BF else 'f32'


def signed(g, n, lo, hi):
    """n values of both signs with magnitude in [lo, hi]"""
    return (torch.rand(n, generator=g) * (hi - lo) + lo) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)


def case_id(c):
    return '-'.join(str(v).replace('torch.', '') for v in c[:-1])


# ================================================================================================ 1. fva_bn_silu_apply (table form)
#  dt  B   H   W    C    res  res_pad z_pad   regime
APPLY_CASES = [
    (BF, 2, 5, 7, 64, True, 1, 1, 'row_chunks 72 < 256: one step, second chunk never valid'),
    (BF, 2, 3, 32, 64, False, 0, 0, 'row_chunks = 256: first chunk full, second wholly invalid'),
    (BF, 2, 4, 45, 64, True, 0, 1, 'row_chunks 376 in (256, 512): second chunk of the step partly valid; odd W'),
    (BF, 1, 3, 75, 64, True, 1, 1, 'row_chunks 616 in (512, 768): second iteration whose second chunk is invalid; B = 1'),
    (BF, 1, 3, 300, 64, True, 1, 0, 'row_chunks 2400 > 2048: five iterations, res_pad 1 with z_pad 0'),
    (BF, 3, 4, 33, 8, True, 1, 1, 'cpp = 1 (C = 8): 35 chunks'),
    (BF, 2, 2, 299, 8, False, 0, 1, 'cpp = 1, row_chunks 301 in (256, 512)'),
    (BF, 1, 1, 5, 1024, True, 0, 1, 'cpp = 128 (C = 1024 bf16), H = 1, B = 1: 896 chunks, two full iterations'),
    (BF, 32, 80, 80, 128, True, 1, 1, 'benchmark shape 32 x 80 x 80 x 128 with residual: 1312 chunks per row; rounding bias'),
    (FP, 1, 1, 3, 1024, False, 0, 0, 'cpp = 256 (C = 1024 fp32, the maximum): a pixel per step, H = 1'),
    (FP, 2, 3, 9, 4, True, 1, 1, 'cpp = 1 (C = 4 fp32)'),
    (FP, 2, 3, 21, 64, True, 1, 1, 'fp32 row_chunks 368 in (256, 512)'),
    (FP, 2, 2, 75, 32, False, 0, 0, 'fp32 row_chunks 600 in (512, 768), no residual: the sigmoid tails carry the whole result'),
    (FP, 1, 2, 70, 128, True, 0, 1, 'fp32 row_chunks 2304 > 2048'),
]


def apply_inputs(dt, B, H, W, Cc, has_res, seed):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(B, H, W, Cc, generator=g) * 1.5 + 0.3).to(dt)
    res = torch.randn(B, H, W, Cc, generator=g).to(dt) if has_res else None
    scale, shift = signed(g, Cc, 0.3, 2.0), torch.rand(Cc, generator=g) * 2 - 1     # u = y * scale + shift spans +-12 and beyond
    scale[Cc // 2] = 0.0
    return y, res, scale, shift


def check_apply(got, y, scale, shift, res, what):
    z64, s64 = sm.silu_apply(y, scale, shift, res, torch.float64)
    z32, _ = sm.silu_apply(y, scale, shift, res, torch.float32)
    mag = s64.abs() if res is None else torch.maximum(s64.abs(), res.double().abs())
    bf = got.dtype == BF
    return sm.check(got, z64, z32, mag, bf, bias=bf and got.numel() >= sm.BIAS_MIN_N, factor=sm.FACTOR_SIGMOID, what=what)


@pytest.mark.parametrize('case', APPLY_CASES, ids=case_id)
def test_bn_silu_apply(case):
    _lib, ops = api()
    dt, B, H, W, Cc, has_res, rp, zp, regime = case
    y, res, scale, shift = apply_inputs(dt, B, H, W, Cc, has_res, 100 + W + Cc)
    if B * H * W * Cc >= 1000000:
        u = y.double() * scale.double() + shift.double()
        assert u.min() < -12 and u.max() > 12
    yd, sd, hd = gpu(y), gpu(scale), gpu(shift)
    rd = gpu(in_halo(res, rp)) if has_res else None
    z = nan_buf((B, H + 2 * zp, W + 2 * zp, Cc), dt)
    _lib.call('fva_bn_silu_apply', ops._code(dt), ops._p(yd), ops._p(sd), ops._p(hd), ops._p(rd), rp, ops._p(z), zp, B, H, W, Cc, ops._stream())
    got = interior(z.cpu(), zp, regime)
    w = check_apply(got, y, scale, shift, res, regime)
    print(f'\n  fva_bn_silu_apply {key(dt)} [{regime}]: worst err / limit {w:.3f}')


def test_bn_silu_apply_refuses_24_channels():
    """C = 24 (bf16): three chunks per pixel do not divide the block -> FVA_ERR_ARG, the output untouched"""
    _lib, ops = api()
    lib = _lib.load()
    y = torch.zeros(1, 2, 2, 24, dtype=BF, device=dev())
    sc = torch.ones(24, device=dev())
    z = nan_buf((1, 4, 4, 24), BF)
    rc = lib.fva_bn_silu_apply(_lib.BF16, ops._p(y), ops._p(sc), ops._p(sc), C.c_void_p(0), 0, ops._p(z), 1, 1, 2, 2, 24, ops._stream())
    torch.cuda.synchronize()
    assert rc == -1 and b'power of two' in lib.fva_last_error()
    assert torch.isnan(z).all()


# ================================================================================================ 2. fva_bn_silu_apply_acc
def fx_words(s):
    """float64 -> the two fixed-point words of the accumulator: hi in units of 2^-8, lo in units of 2^-56 (both exact scalings)"""
    hi = torch.round(s * 256.0)
    lo = torch.round((s - hi / 256.0) * 2.0 ** 56)
    return hi.to(torch.int64), lo.to(torch.int64)


def fx_value(h, l):
    return h.double() * (1.0 / 256.0) + l.double() * 2.0 ** -56


def fill_acc(s1, s2, R, g):
    """int64 [R][5][C] whose copies add up to the words of s1 / s2, spread unevenly; returns (acc, the values the kernel will read)"""
    Cc = s1.numel()
    h1, l1 = fx_words(s1)
    h2, l2 = fx_words(s2)
    acc = torch.zeros(R, 5, Cc, dtype=torch.int64)
    for k, wd in enumerate((h1, h2, l1, l2)):
        rest = wd.clone()
        for r in range(R - 1):
            part = torch.randint(-2 ** 40, 2 ** 40, (Cc,), generator=g, dtype=torch.int64) if r % 2 == 0 else torch.zeros(Cc, dtype=torch.int64)
            acc[r, k] = part
            rest -= part
        acc[R - 1, k] = rest
    return acc, fx_value(h1, l1), fx_value(h2, l2)


#  dt  B   H   W   C   res  res_pad z_pad replicas   regime
APPLY_ACC_CASES = [
    (BF, 2, 6, 20, 64, False, 0, 1, 1, '16 rows < 2048 blocks, row_chunks 176 < 256: threads that load nothing in the prologue'),
    (BF, 2, 4, 75, 64, True, 1, 1, 4, 'row_chunks 616: the prologue load feeds the first step only; four replicas through LDS'),
    (FP, 3, 9, 11, 32, True, 0, 0, 4, 'fp32, pads 0, four replicas'),
    (BF, 32, 80, 80, 64, True, 1, 1, 4, '2624 padded rows > 2048 blocks: blocks 0..575 walk two rows, some start on a border row; rounding bias'),
]


@pytest.mark.parametrize('case', APPLY_ACC_CASES, ids=case_id)
def test_bn_silu_apply_acc(case):
    _lib, ops = api()
    dt, B, H, W, Cc, has_res, rp, zp, R, regime = case
    g = torch.Generator().manual_seed(7 + W)
    y = (torch.randn(B, H, W, Cc, generator=g) * (torch.rand(Cc, generator=g) + 0.5) + torch.randn(Cc, generator=g)).to(dt)
    res = torch.randn(B, H, W, Cc, generator=g).to(dt) if has_res else None
    gamma, beta = signed(g, Cc, 0.3, 3.0), torch.rand(Cc, generator=g) * 2 - 1
    M, eps, mom = B * H * W, 1e-5, 0.1
    yd64 = y.double().reshape(M, Cc)
    acc, s1, s2 = fill_acc(yd64.sum(0), (yd64 * yd64).sum(0), R, g)
    rm0, rv0 = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    accd, zero = gpu(acc), torch.ones(R * 5 * Cc, dtype=torch.int64, device=dev())
    rm, rv, nbt = gpu(rm0), gpu(rv0), torch.full((1,), 41, dtype=torch.int64, device=dev())
    gd, bd = gpu(gamma), gpu(beta)
    mean, rstd, scale, shift = (nan_buf((Cc,), FP) for _ in range(4))
    fin = _lib.BnFwdAcc(accd.data_ptr(), zero.data_ptr(), R, gd.data_ptr(), bd.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), mom, eps,
                        mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(), shift.data_ptr())
    yd = gpu(y)
    rd = gpu(in_halo(res, rp)) if has_res else None
    z = nan_buf((B, H + 2 * zp, W + 2 * zp, Cc), dt)
    _lib.call('fva_bn_silu_apply_acc', ops._code(dt), ops._p(yd), C.byref(fin), ops._p(rd), rp, ops._p(z), zp, B, H, W, Cc, ops._stream())
    torch.cuda.synchronize()
    # the statistics against float64 (the tolerances of test_bn_finalize_large_tables)
    m = s1 / M
    var = (s2 / M - m * m).clamp_min(0)
    r = 1 / torch.sqrt(var + eps)
    assert torch.allclose(mean.cpu().double(), m, rtol=2e-6, atol=1e-7)
    assert torch.allclose(rstd.cpu().double(), r, rtol=2e-5)
    assert torch.allclose(scale.cpu().double(), gamma.double() * r, rtol=2e-5)
    assert torch.allclose(shift.cpu().double(), beta.double() - m * gamma.double() * r, rtol=2e-5, atol=2e-5 * (m * gamma.double() * r).abs().max().item())
    assert torch.allclose(rm.cpu().double(), (1 - mom) * rm0.double() + mom * m, rtol=2e-6, atol=1e-7)
    assert torch.allclose(rv.cpu().double(), (1 - mom) * rv0.double() + mom * var * M / (M - 1), rtol=2e-5)
    assert int(nbt) == 42
    assert not zero.any(), '`zero` comes back all-zero'
    assert torch.equal(accd.cpu(), acc), 'the accumulator this launch reads stays as it is'
    # z from the coefficients the kernel itself wrote out (every block computes the same bits)
    got = interior(z.cpu(), zp, regime)
    w = check_apply(got, y, scale.cpu(), shift.cpu(), res, regime)
    print(f'\n  fva_bn_silu_apply_acc {key(dt)} [{regime}]: worst err / limit {w:.3f}')


# ================================================================================================ 3. fva_bn_silu_bwd_reduce / _acc
#  dt   M     C      regime (rpi = 256 / cpp pixel rows per block step; a block owns max(ceil(M / 2048), 8 * rpi) rows, rounded up to rpi)
REDUCE_CASES = [
    (FP, 37, 1024, 'cpp = 256, rpi = 1: 8 rows per block, M = 37 not a multiple'),
    (BF, 300, 8, 'cpp = 1, rpi = 256: M = 300 smaller than one block\'s 2048 rows'),
    (BF, 5000, 8, 'cpp = 1: 3 blocks, the last one short'),
    (FP, 2048 * 2 + 5, 4, 'fp32 cpp = 1: 3 blocks, the last holds 5 rows (255 of its 256 row groups idle)'),
    (BF, 1000, 64, 'cpp = 8, rpi = 32: 256 rows per block, M not a multiple'),
    (BF, 32 * 80 * 80, 128, 'benchmark layer M = 204800, C = 128: rpi = 16, 1600 blocks of 128 rows'),
]


def reduce_inputs(dt, M, Cc, seed):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(M, Cc, generator=g) * 1.5 + 0.3).to(dt)
    dz = torch.randn(M, Cc, generator=g).to(dt)
    scale, shift = signed(g, Cc, 0.3, 2.0), torch.rand(Cc, generator=g) * 2 - 1
    mean, rstd = torch.randn(Cc, generator=g) * 0.5 + 0.3, torch.rand(Cc, generator=g) + 0.4
    return y, dz, scale, shift, mean, rstd


def reduce_reference(dz, y, scale, shift, mean, rstd, n):
    """float64 sums [2][C] of dU and dU * xhat, and their limit"""
    t64 = sm.bwd_terms(dz, y, scale, shift, mean, rstd, torch.float64)
    t32 = sm.bwd_terms(dz, y, scale, shift, mean, rstd, torch.float32)
    ref = torch.stack([t.sum(0) for t in t64])
    lim = torch.stack([sm.sum_limit(n, a.abs().sum(0), (b.double() - a).abs().sum(0)) for a, b in zip(t64, t32)])
    return ref, lim


@pytest.mark.parametrize('case', REDUCE_CASES, ids=case_id)
def test_bn_silu_bwd_reduce(case):
    _lib, ops = api()
    lib = _lib.load()
    dt, M, Cc, regime = case
    y, dz, scale, shift, mean, rstd = reduce_inputs(dt, M, Cc, M % 997)
    nb = lib.fva_bn_bwd_blocks(ops._code(dt), M, Cc)
    assert nb > 0
    n = -(-M // nb)                       # the longest chain of fp32 additions behind one table entry
    ref, lim = reduce_reference(dz, y, scale, shift, mean, rstd, n)
    dev_in = [gpu(t) for t in (dz, y, scale, shift, mean, rstd)]
    part = nan_buf((nb, 2, Cc), FP)
    _lib.call('fva_bn_silu_bwd_reduce', ops._code(dt), *[ops._p(t) for t in dev_in], ops._p(part), nb, M, Cc, ops._stream())
    got = part.cpu().double().sum(0)
    w = ((got - ref).abs() / lim).max().item()
    assert torch.isfinite(got).all() and w <= 1.0, f'{regime}: worst err / limit {w:.3f}'
    msg = f'\n  fva_bn_silu_bwd_reduce {key(dt)} [{regime}]: worst err / limit {w:.3f}'
    # the accumulator form: the same partials split exactly into integers; the host adds the copies
    for R in (1, 8):
        words = []
        for _ in range(2):
            acc = torch.zeros(R, 5, Cc, dtype=torch.int64, device=dev())
            _lib.call('fva_bn_silu_bwd_reduce_acc', ops._code(dt), *[ops._p(t) for t in dev_in], ops._p(acc), R, M, Cc, ops._stream())
            words.append(acc.cpu())
        assert torch.equal(words[0], words[1]), 'a second run gives the same words'
        a = words[0].sum(0)
        assert not a[4].any()
        if R == 8 and nb >= 8:
            assert all(words[0][r].any() for r in range(R)), 'block b adds to copy b mod replicas'
        got = torch.stack([fx_value(a[0], a[2]), fx_value(a[1], a[3])])
        wa = ((got - ref).abs() / lim).max().item()
        assert wa <= 1.0, f'{regime} (acc, {R} replicas): worst err / limit {wa:.3f}'
        msg += f'; acc x{R} {wa:.3f}'
    print(msg)


# ================================================================================================ 4. fva_bn_bwd_finalize + fva_bn_silu_bwd_apply, and _apply_acc
#  dt  B   H   W    C   dy_pad replicas  regime (the row regimes of groups 1 and 2)
BWD_APPLY_CASES = [
    (BF, 2, 5, 7, 64, 1, 1, 'row_chunks 72 < 256'),
    (BF, 2, 3, 32, 64, 0, 1, 'row_chunks = 256'),
    (BF, 2, 4, 45, 64, 1, 4, 'row_chunks 376 in (256, 512), odd W'),
    (BF, 1, 3, 75, 64, 1, 8, 'row_chunks 616 in (512, 768), B = 1'),
    (BF, 1, 3, 300, 64, 0, 1, 'row_chunks 2400 > 2048'),
    (BF, 3, 4, 33, 8, 1, 2, 'cpp = 1'),
    (BF, 1, 1, 5, 1024, 1, 2, 'cpp = 128, H = 1, B = 1'),
    (FP, 1, 1, 3, 1024, 0, 1, 'cpp = 256 fp32'),
    (FP, 2, 3, 21, 64, 1, 4, 'fp32 row_chunks 368'),
    (FP, 2, 2, 75, 32, 0, 1, 'fp32 row_chunks 600 in (512, 768)'),
    (BF, 32, 80, 80, 64, 1, 4, '2624 padded rows: the accumulator form walks two rows per block; rounding bias'),
]


def check_coef(got, ref64, what):
    """a per-channel fp32 output that is at most three fp32 roundings away from its float64 value"""
    assert ((got.double() - ref64).abs() <= 4 * sm.EPS32 * ref64.abs()).all(), what


@pytest.mark.parametrize('case', BWD_APPLY_CASES, ids=case_id)
def test_bn_bwd_finalize_and_apply(case):
    _lib, ops = api()
    lib = _lib.load()
    dt, B, H, W, Cc, pad, R, regime = case
    M = B * H * W
    y, dz, scale, shift, mean, rstd = reduce_inputs(dt, M, Cc, 31 + W + Cc)
    g = torch.Generator().manual_seed(5)
    gamma = signed(g, Cc, 0.5, 1.5)
    t64 = sm.bwd_terms(dz, y, scale, shift, mean, rstd, torch.float64)
    S = torch.stack([t.sum(0) for t in t64])                                        # realistic sums: those of these very inputs
    dev_in = [gpu(t) for t in (dz, y, scale, shift, mean, rstd)]
    gd = gpu(gamma)
    y4, dz4 = y.view(B, H, W, Cc), dz.view(B, H, W, Cc)
    bf = dt == BF
    msg = ''
    for accumulate in (0, 1):
        pre_g, pre_b = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
        # ---- table form: a three-row table whose float64 column sums are what the finalize pass reads (summed in double: exact)
        nb = 3
        rows = lib.fva_bn_partial_rows(nb)
        table = (S[None] * torch.tensor([0.5, 0.3, 0.2], dtype=torch.float64)[:, None, None]).float()
        T = table.double().sum(0)
        part = gpu(table)
        dgamma, dbeta, coef = gpu(pre_g), gpu(pre_b), nan_buf((3, Cc), FP)
        _lib.call('fva_bn_bwd_finalize', ops._p(part), nb, rows, M, Cc, ops._p(gd), ops._p(dev_in[5]), ops._p(dgamma), ops._p(dbeta), accumulate, ops._p(coef), ops._stream())
        cf = coef.cpu()
        a64 = gamma.double() * rstd.double()
        check_coef(cf[0], a64, 'coef a')
        check_coef(cf[1], -a64 * T[1] / M, 'coef b')
        check_coef(cf[2], -a64 * T[0] / M, 'coef c')
        for got, t, pre, name in ((dgamma, T[1], pre_g, 'dgamma'), (dbeta, T[0], pre_b, 'dbeta')):
            want = t + (pre.double() if accumulate else 0)
            assert ((got.cpu().double() - want).abs() <= 2 * sm.EPS32 * (t.abs() + pre.double().abs() * accumulate)).all(), (name, accumulate)
        dy = nan_buf((B, H + 2 * pad, W + 2 * pad, Cc), dt)
        _lib.call('fva_bn_silu_bwd_apply', ops._code(dt), *[ops._p(t) for t in dev_in], ops._p(coef), ops._p(dy), pad, B, H, W, Cc, ops._stream())
        got = interior(dy.cpu(), pad, regime)
        r64, mag = sm.bwd_apply(dz4, y4, scale, shift, mean, rstd, cf[0], cf[1], cf[2], torch.float64)
        r32, _ = sm.bwd_apply(dz4, y4, scale, shift, mean, rstd, cf[0], cf[1], cf[2], torch.float32)
        w = sm.check(got, r64, r32, mag, bf, bias=bf and got.numel() >= sm.BIAS_MIN_N, factor=sm.FACTOR_SIGMOID, what=regime)
        # ---- accumulator form: the sums arrive as fixed-point words, the coefficients are made in the kernel's prologue (the arithmetic of
        # bn_bwd_coef, restated here in the same precision: a = gamma * rstd in fp32, the other two in double and rounded once)
        acc, v1, v2 = fill_acc(S[0], S[1], R, g)
        accd, zero = gpu(acc), torch.ones(R * 5 * Cc, dtype=torch.int64, device=dev())
        dgamma, dbeta = gpu(pre_g), gpu(pre_b)
        desc = _lib.BnBwdAcc(accd.data_ptr(), zero.data_ptr(), R, gd.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), accumulate)
        dy = nan_buf((B, H + 2 * pad, W + 2 * pad, Cc), dt)
        _lib.call('fva_bn_silu_bwd_apply_acc', ops._code(dt), *[ops._p(t) for t in dev_in], C.byref(desc), ops._p(dy), pad, B, H, W, Cc, ops._stream())
        torch.cuda.synchronize()
        a32 = gamma * rstd
        inv = 1.0 / M
        cb, cc = (-a32.double() * v2 * inv).float(), (-a32.double() * v1 * inv).float()
        for got, t, pre, name in ((dgamma, v2, pre_g, 'dgamma'), (dbeta, v1, pre_b, 'dbeta')):
            want = t + (pre.double() if accumulate else 0)
            assert ((got.cpu().double() - want).abs() <= 2 * sm.EPS32 * (t.abs() + pre.double().abs() * accumulate)).all(), (name, accumulate, 'acc')
        assert not zero.any() and torch.equal(accd.cpu(), acc)
        got = interior(dy.cpu(), pad, regime)
        r64, mag = sm.bwd_apply(dz4, y4, scale, shift, mean, rstd, a32, cb, cc, torch.float64)
        r32, _ = sm.bwd_apply(dz4, y4, scale, shift, mean, rstd, a32, cb, cc, torch.float32)
        wa = sm.check(got, r64, r32, mag, bf, bias=bf and got.numel() >= sm.BIAS_MIN_N, factor=sm.FACTOR_SIGMOID, what=regime + ' (acc)')
        msg += f' accumulate={accumulate}: table {w:.3f}, acc x{R} {wa:.3f};'
        if M * Cc > 1000000 and accumulate == 0:
            break                                                   # the large shape once (accumulate only touches [C] vectors)
    print(f'\n  fva_bn_silu_bwd_apply {key(dt)} [{regime}]: worst err / limit{msg}')


def test_bn_silu_block_backward_against_float64_autograd():
    """reduce -> finalize -> apply (fp32) against float64 autograd of silu(batch_norm(y)) + res.  Beyond the element measure (e32 = the same
    autograd in fp32 on the CPU) the chain is allowed what its statistics may be off by, derived: the two sums by the sum rule
    ((n + 2) * 2^-24 * sum|term| each, entering dY as a * (d1 + |xhat| d2) / M), and u = y * scale + shift from fp32 coefficients that are
    themselves rounded (|du| <= 4 * 2^-24 * (|y scale| + |mean scale| + |beta|), entering through |dz| * max|SiLU''| = |dz| / 2)."""
    _lib, ops = api()
    lib = _lib.load()
    B, H, W, Cc, eps = 3, 10, 75, 32, 1e-5                          # fp32 row_chunks 600: second iteration with an invalid second chunk
    M = B * H * W
    g = torch.Generator().manual_seed(77)
    y = torch.randn(B, H, W, Cc, generator=g) * (torch.rand(Cc, generator=g) + 0.5) + torch.randn(Cc, generator=g)
    dz = torch.randn(B, H, W, Cc, generator=g)
    gamma, beta = signed(g, Cc, 0.5, 2.5), torch.rand(Cc, generator=g) * 2 - 1

    def autograd(dt):
        yy = y.to(dt).permute(0, 3, 1, 2).clone().requires_grad_(True)
        z = F.silu(F.batch_norm(yy, None, None, gamma.to(dt), beta.to(dt), True, 0.0, eps))     # (+ res: its gradient is dz itself)
        z.backward(dz.to(dt).permute(0, 3, 1, 2))
        return yy.grad.permute(0, 2, 3, 1).contiguous()

    r64, r32 = autograd(torch.float64), autograd(torch.float32)
    y64 = y.double().reshape(M, Cc)
    m64 = y64.mean(0)
    rs64 = 1 / torch.sqrt(y64.var(0, unbiased=False) + eps)
    mean, rstd = m64.float(), rs64.float()                          # what the forward pass leaves: rounded once
    scale = gamma * rstd
    shift = beta - mean * scale
    dev_in = [gpu(t) for t in (dz, y, scale, shift, mean, rstd)]
    gd = gpu(gamma)
    nb = lib.fva_bn_bwd_blocks(_lib.F32, M, Cc)
    rows = lib.fva_bn_partial_rows(nb)
    part = nan_buf((rows, 2, Cc), FP)
    dgamma, dbeta, coef = (nan_buf((Cc,), FP), nan_buf((Cc,), FP), nan_buf((3, Cc), FP))
    dy = nan_buf((B, H + 2, W + 2, Cc), FP)
    _lib.call('fva_bn_silu_bwd_reduce', _lib.F32, *[ops._p(t) for t in dev_in], ops._p(part), nb, M, Cc, ops._stream())
    _lib.call('fva_bn_bwd_finalize', ops._p(part), nb, rows, M, Cc, ops._p(gd), ops._p(dev_in[5]), ops._p(dgamma), ops._p(dbeta), 0, ops._p(coef), ops._stream())
    _lib.call('fva_bn_silu_bwd_apply', _lib.F32, *[ops._p(t) for t in dev_in], ops._p(coef), ops._p(dy), 1, B, H, W, Cc, ops._stream())
    got = interior(dy.cpu(), 1)
    du, dux = sm.bwd_terms(dz, y, scale, shift, mean, rstd, torch.float64)
    a = (gamma.double() * rs64).abs()
    n = -(-M // nb)
    d1, d2 = (n + 2) * sm.EPS32 * du.abs().sum((0, 1, 2)), (n + 2) * sm.EPS32 * dux.abs().sum((0, 1, 2))
    xhat = (y.double() - m64) * rs64
    dudev = 4 * sm.EPS32 * ((y.double() * scale.double()).abs() + (m64 * scale.double()).abs() + beta.double().abs())
    extra = a * ((d1 + xhat.abs() * d2) / M + dz.double().abs() * 0.5 * dudev)
    _, mag = sm.bwd_apply(dz, y, scale, shift, mean, rstd, gamma.double() * rs64, -a * dux.sum((0, 1, 2)) / M, -a * du.sum((0, 1, 2)) / M, torch.float64)
    lim = sm.limit_of(r64, r32, mag, sm.FACTOR_SIGMOID) + extra
    w = sm.worst_f32(got, r64, lim)
    assert w <= 1.0, w
    assert ((dbeta.cpu().double() - du.sum((0, 1, 2))).abs() <= d1 + 4 * (sm.bwd_terms(dz, y, scale, shift, mean, rstd, torch.float32)[0].double() - du).abs().sum((0, 1, 2))).all()
    print(f'\n  reduce -> finalize -> apply against float64 autograd: worst err / limit {w:.3f}')


# ================================================================================================ 5. statistics of a channel with a large mean
def test_statistics_of_a_channel_with_a_large_mean():
    """fp32 1x1 convolution with one constant input channel and a large weight: y = m + noise, m / std in {0, 10, 100}.  The statistics are
    fp32 sums of y and y^2 per tile, so the variance loses mean^2 / var in precision where nn.BatchNorm2d (two-pass / Welford) does not.
    Asserted is what is derivable, against float64 statistics of the downloaded fp32 y (the very accumulators the sums were taken from):
    |var_got - var| <= 257 * 2^-24 * E[y^2] (256 = the tallest tile, any order), var_got >= 0, rstd finite.  var_got is read back through
    the running variance with momentum 1 (the unbiased variance, rounded to fp32 once).  The realised relative error of rstd is REPORTED."""
    _lib, ops = api()
    lib = _lib.load()
    B, Cin, N, H, eps = 2, 64, 64, 16, 1e-5
    M = B * H * H
    report = []
    for ratio in (0.0, 10.0, 100.0):
        g = torch.Generator().manual_seed(9)
        x = torch.zeros(B, H + 2, H + 2, Cin)
        x[:, 1:-1, 1:-1] = torch.randn(B, H, H, Cin, generator=g)
        x[:, 1:-1, 1:-1, 0] = 1.0
        w = torch.randn(N, Cin, 1, 1, generator=g) / (Cin - 1) ** 0.5
        w[:, 0] = ratio
        d = _lib.ConvDesc(_lib.F32, B, H, H, Cin, N, 1, 1, 1, 1)
        wf, _ = ops.packed_weights(gpu(w), d, FP, cache=False)
        nblk = lib.fva_conv_stat_blocks(C.byref(d))
        rows = lib.fva_bn_partial_rows(nblk)
        part = nan_buf((rows, 2, N), FP)
        y = nan_buf((M, N), FP)
        xd = gpu(x)
        _lib.call('fva_conv_fwd', C.byref(d), ops._p(xd), ops._p(wf), ops._p(y), ops._p(part), ops._stream())
        gamma, beta = torch.ones(N, device=dev()), torch.zeros(N, device=dev())
        rm, rv = torch.zeros(N, device=dev()), torch.ones(N, device=dev())
        mean, rstd, scale, shift = (nan_buf((N,), FP) for _ in range(4))
        _lib.call('fva_bn_finalize', ops._p(part), nblk, rows, M, N, ops._p(gamma), ops._p(beta), ops._p(rm), ops._p(rv), C.c_void_p(0), 1.0, eps,
                  ops._p(mean), ops._p(rstd), ops._p(scale), ops._p(shift), ops._stream())
        yd = y.cpu().double()
        assert torch.isfinite(yd).all()
        var = yd.var(0, unbiased=False)
        ey2 = (yd * yd).mean(0)
        std_ratio = (yd.mean(0).abs() / var.sqrt()).median().item()
        var_got = rv.cpu().double() * (M - 1) / M
        assert (var_got >= 0).all() and torch.isfinite(rstd).all()
        werr = ((var_got - var).abs() / (257 * sm.EPS32 * ey2)).max().item()
        assert werr <= 1.0, (ratio, werr)
        rel = ((rstd.cpu().double() - 1 / torch.sqrt(var + eps)).abs() * torch.sqrt(var + eps)).max().item()
        report.append(f'm/std {std_ratio:.1f}: var err / bound {werr:.4f}, rstd relative error {rel:.2e}')
    print('\n  large-mean statistics (sum / sum-of-squares form): ' + '; '.join(report))


# ================================================================================================ 6. fva_upsample2_concat_fwd / _bwd
#  dt  B  h   w   Cup  Cskip up_pad skip_pad up_first   regime
UPCAT_CASES = [
    (BF, 1, 3, 5, 8, 8, 0, 0, 1, 'one chunk per tensor, odd h and w, B = 1, pads 0 / 0'),
    (BF, 3, 5, 3, 64, 32, 1, 0, 0, 'skip first, up_pad 1 / skip_pad 0, B = 3'),
    (BF, 3, 4, 7, 64, 32, 0, 1, 1, 'up first, up_pad 0 / skip_pad 1'),
    (FP, 1, 3, 5, 8, 8, 1, 1, 0, 'fp32 (4 elements per chunk), pads 1 / 1, skip first'),
    (FP, 3, 2, 3, 64, 32, 1, 1, 1, 'fp32, up first'),
    (BF, 32, 20, 20, 256, 512, 1, 1, 1, 'benchmark 32 x 20 x 20 (256, 512): 5.4M chunks forward, 3.7M items backward -> the grid-stride loops run more than once'),
    (BF, 32, 20, 20, 256, 512, 1, 1, 0, 'the same, skip first (the channel offset of both sources changes)'),
]


@pytest.mark.parametrize('case', UPCAT_CASES, ids=case_id)
def test_upsample2_concat(case):
    _lib, ops = api()
    dt, B, h, w, Cu, Cs, up_pad, sk_pad, up_first, regime = case
    g = torch.Generator().manual_seed(h * 100 + w)
    up = torch.randn(B, h, w, Cu, generator=g).to(dt)
    skip = torch.randn(B, 2 * h, 2 * w, Cs, generator=g).to(dt)
    upd, skd = gpu(in_halo(up, up_pad)), gpu(in_halo(skip, sk_pad))
    out = nan_buf((B, 2 * h + 2, 2 * w + 2, Cu + Cs), dt)
    _lib.call('fva_upsample2_concat_fwd', ops._code(dt), ops._p(upd), up_pad, ops._p(skd), sk_pad, ops._p(out), B, h, w, Cu, Cs, up_first, ops._stream())
    got = interior(out.cpu(), 1, regime)
    up2 = up.repeat_interleave(2, 1).repeat_interleave(2, 2)
    want = torch.cat([up2, skip] if up_first else [skip, up2], 3)
    assert torch.equal(bits(got), bits(want)), f'{regime}: the forward pass is a copy'
    # backward
    dcat = torch.randn(B, 2 * h, 2 * w, Cu + Cs, generator=g).to(dt)
    dd = gpu(dcat)
    dup, dsk = nan_buf((B, h, w, Cu), dt), nan_buf((B, 2 * h, 2 * w, Cs), dt)
    _lib.call('fva_upsample2_concat_bwd', ops._code(dt), ops._p(dd), ops._p(dup), ops._p(dsk), B, h, w, Cu, Cs, up_first, ops._stream())
    uo, so = (0, Cu) if up_first else (Cs, 0)
    assert torch.equal(bits(dsk.cpu()), bits(dcat[..., so:so + Cs])), f'{regime}: dskip is a copy'
    v = dcat[..., uo:uo + Cu].reshape(B, h, 2, w, 2, Cu).permute(0, 1, 3, 5, 2, 4).reshape(B, h, w, Cu, 4)      # (dy, dx) in the kernel's order
    r64 = v.double().sum(-1)
    vf = v.float()
    r32 = ((vf[..., 0] + vf[..., 1]) + vf[..., 2]) + vf[..., 3]
    bf = dt == BF
    wst = sm.check(dup.cpu(), r64, r32, v.double().abs().sum(-1), bf, bias=bf and r64.numel() >= sm.BIAS_MIN_N, what=regime)
    print(f'\n  fva_upsample2_concat {key(dt)} [{regime}]: forward and dskip bit-exact, dup worst err / limit {wst:.3f}')


# ================================================================================================ 7. fva_pack_nchw / fva_cast_nhwc
def specials(t):
    """plant +-Inf, -0.0, NaN and values exactly halfway between two bf16 numbers (ties go to the even neighbour, down and up)"""
    f = t.view(-1)
    vals = [float('inf'), float('-inf'), -0.0, NAN, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 3.3895313892515355e38]
    for i, v in enumerate(vals):                # one element in 13, all over the tensor: every view of it holds each of them
        f[i * 13::13 * len(vals)] = v
    return t


def same_bits(got, want, what):
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    assert torch.equal(nan_g, nan_w), f'{what}: NaN stays NaN, and only NaN'
    assert torch.equal(bits(got)[~nan_w], bits(want)[~nan_w]), what


def halo_expect(nhwc, dt, pad):
    B, H, W, Cc = nhwc.shape
    out = torch.zeros(B, H + 2 * pad, W + 2 * pad, Cc, dtype=dt)
    out[:, pad:pad + H, pad:pad + W] = nhwc.to(dt)          # torch's own cast: round to nearest even
    return out


@pytest.mark.parametrize('Cc', [3, 8, 255])
@pytest.mark.parametrize('sdt,ddt', [(FP, FP), (FP, BF), (BF, FP), (BF, BF)], ids=['f32-f32', 'f32-bf16', 'bf16-f32', 'bf16-bf16'])
def test_pack_nchw(sdt, ddt, Cc):
    """sources: contiguous NCHW; channels-last; a sliced view with a storage offset; a batch-expanded view (stride 0); dst_pad 0 and 1"""
    _lib, ops = api()
    B, H, W = 3, 5, 7
    g = torch.Generator().manual_seed(Cc)
    base = specials(torch.randn(B, Cc + 2, H + 3, W + 2, generator=g).to(sdt))
    based = gpu(base)
    views = {
        'contiguous': lambda t: t[:, :Cc, :H, :W].contiguous(),
        'channels_last': lambda t: t[:, :Cc, :H, :W].contiguous(memory_format=torch.channels_last),
        'sliced': lambda t: t[:, 1:1 + Cc, 2:2 + H, 1:1 + W],
        'expanded': lambda t: t[1:2, 2:2 + Cc, 1:1 + H, :W].expand(B, Cc, H, W),
    }
    for name, view in views.items():
        src, srcd = view(base), view(based)
        assert src.stride() == srcd.stride() or name in ('contiguous', 'channels_last')
        if name == 'sliced':
            assert srcd.storage_offset() > 0
        if name == 'expanded':
            assert srcd.stride(0) == 0
        for pad in (0, 1):
            dst = nan_buf((B, H + 2 * pad, W + 2 * pad, Cc), ddt)
            sb, sc, sh, sw = srcd.stride()
            _lib.call('fva_pack_nchw', ops._code(ddt), ops._p(srcd), 1 if sdt == BF else 0, sb, sc, sh, sw, ops._p(dst), pad, B, Cc, H, W, ops._stream())
            same_bits(dst.cpu(), halo_expect(src.permute(0, 2, 3, 1), ddt, pad), f'pack {name} pad {pad}')


@pytest.mark.parametrize('Cc', [3, 8, 255])
@pytest.mark.parametrize('sdt,ddt', [(FP, FP), (FP, BF), (BF, FP), (BF, BF)], ids=['f32-f32', 'f32-bf16', 'bf16-f32', 'bf16-bf16'])
def test_cast_nhwc(sdt, ddt, Cc):
    """pads 0 -> 1, 1 -> 0, 1 -> 1, 0 -> 0; the source border is NaN (never read), the destination border +0"""
    _lib, ops = api()
    B, H, W = 2, 6, 5
    g = torch.Generator().manual_seed(Cc + 1)
    src = specials(torch.randn(B, H, W, Cc, generator=g).to(sdt))
    for sp, dp in ((0, 1), (1, 0), (1, 1), (0, 0)):
        srcd = gpu(in_halo(src, sp))
        dst = nan_buf((B, H + 2 * dp, W + 2 * dp, Cc), ddt)
        _lib.call('fva_cast_nhwc', ops._p(srcd), ops._code(sdt), sp, ops._p(dst), ops._code(ddt), dp, B, H, W, Cc, ops._stream())
        same_bits(dst.cpu(), halo_expect(src, ddt, dp), f'cast pads {sp} -> {dp}')


# ================================================================================================ 8. fva_bn_eval_coeffs
@pytest.mark.parametrize('Cc', [1, 255, 1024])
def test_bn_eval_coeffs(Cc):
    _lib, ops = api()
    g = torch.Generator().manual_seed(Cc)
    gamma, beta, rm = signed(g, Cc, 0.1, 2.0), torch.randn(Cc, generator=g), torch.randn(Cc, generator=g) * 3
    rv = torch.rand(Cc, generator=g) * 4
    rv[0] = 0.0
    if Cc > 1:
        rv[1] = 1e-12
    eps = 1e-5
    scale, shift = nan_buf((Cc,), FP), nan_buf((Cc,), FP)
    ins = [gpu(t) for t in (gamma, beta, rm, rv)]
    _lib.call('fva_bn_eval_coeffs', Cc, *[ops._p(t) for t in ins], eps, ops._p(scale), ops._p(shift), ops._stream())

    def formula(dt):
        e = torch.tensor(eps, dtype=torch.float32).to(dt)           # the kernel receives eps as a float
        sc = gamma.to(dt) / torch.sqrt(rv.to(dt) + e)
        return sc, beta.to(dt) - rm.to(dt) * sc
    (sc64, sh64), (sc32, sh32) = formula(torch.float64), formula(torch.float32)
    w1 = sm.check(scale.cpu(), sc64, sc32, sc64.abs(), False, what='scale')
    w2 = sm.check(shift.cpu(), sh64, sh32, torch.maximum(beta.double().abs(), (rm.double() * sc64).abs()), False, what='shift')
    print(f'\n  fva_bn_eval_coeffs C = {Cc}: worst err / limit scale {w1:.3f}, shift {w2:.3f}')


# ================================================================================================ 9. fva_head_bwd_prepare, fva_head_fwd
#  dt  B   H   W   N   Npad   regime
HEAD_CASES = [
    (BF, 2, 5, 7, 255, 256, 'N = 255 as the product pads it (cpp = 32): the bias sums ride in the repack pass; M = 70'),
    (FP, 1, 9, 9, 75, 128, 'N = 75 -> 128 (cpp = 16), rider, fp32 dy'),
    (BF, 3, 4, 5, 18, 64, 'N = 18 -> 64 (cpp = 8), rider: chunks 3..7 of a pixel are all padding'),
    (FP, 2, 6, 5, 75, 80, 'Npad = 80 (cpp = 10 does not divide 256): the bias partial sums by a launch of their own'),
    (BF, 1, 7, 3, 18, 24, 'Npad = 24 (cpp = 3): separate partial launch, one row block'),
    (BF, 2, 33, 33, 18, 24, 'Npad = 24, M = 2178: separate partial launch with 35 blocks of 63 rows, the last one short'),
    (BF, 32, 80, 80, 255, 256, 'benchmark head 32 x 80 x 80, N = 255: 6.9M items > 4096 x 256 -> the rider\'s grid-stride loop; a thread keeps its chunk'),
]


@pytest.mark.parametrize('case', HEAD_CASES, ids=case_id)
def test_head_bwd_prepare(case):
    _lib, ops = api()
    dt, B, H, W, N, Npad, regime = case
    M = B * H * W
    g = torch.Generator().manual_seed(N + W)
    dhead = torch.randn(M, N, generator=g)
    dd = gpu(dhead)
    ws = nan_buf((4096 * N,), FP)
    cpp = Npad // 8
    items = B * (H + 2) * (W + 2) * cpp
    if 256 % cpp == 0:          # rider: a thread adds its items, then 256 / cpp threads are folded
        n = -(-items // (min(-(-items // 256), 4096) * 256)) + 256 // cpp
    else:                       # separate launch: one thread adds the rows of its block one after the other
        nb = min(-(-M // 64), 1024)
        n = -(-M // nb)
    colsum, colabs = dhead.double().sum(0), dhead.double().abs().sum(0)
    big = M * N > 10000000
    worst = 0.0
    for gs, accumulate in ((None, 0), (1.0, 1), (0.37, 0), (0.37, 1)):
        if big and (gs, accumulate) not in ((None, 0), (0.37, 1)):
            continue
        gsd = None if gs is None else torch.tensor([gs], device=dev())
        gval = torch.tensor(1.0 if gs is None else gs)                    # fp32, as the kernel reads it
        pre = torch.randn(N, generator=g)
        dbias = gpu(pre) if accumulate else nan_buf((N,), FP)
        dy = nan_buf((B, H + 2, W + 2, Npad), dt)
        _lib.call('fva_head_bwd_prepare', ops._code(dt), ops._p(dd), ops._p(gsd), ops._p(dy), ops._p(dbias), accumulate, ops._p(ws), B, H, W, N, Npad, ops._stream())
        got = interior(dy.cpu(), 1, regime)
        assert not bits(got[..., N:]).any(), 'pad columns N..Npad-1 are +0'
        want = (gval * dhead).view(B, H, W, N)                             # the exact fp32 product
        assert torch.equal(bits(got[..., :N]), bits(want.to(dt))), f'{regime}: dy (grad_scale {gs})'
        # dbias = (fp32 of the double sum of the fp32 partials) * g (+ what was there): the sum rule, the factor applied to both sides,
        # and one more rounding each for the product and the accumulation
        ref = colsum * gval.double() + (pre.double() if accumulate else 0)
        lim = sm.sum_limit(n, colabs) * gval.double().abs()
        lim = lim + accumulate * sm.EPS32 * (ref.abs() + lim)
        err = (dbias.cpu().double() - ref).abs()
        assert torch.isfinite(err).all()
        worst = max(worst, (err / lim).max().item())
        assert worst <= 1.0, f'{regime}: dbias (grad_scale {gs}, accumulate {accumulate}) worst err / limit {worst:.3f}'
    print(f'\n  fva_head_bwd_prepare {key(dt)} [{regime}]: dy bit-exact, dbias worst err / limit {worst:.4f} (n = {n})')


@pytest.mark.parametrize('dt', [FP, BF], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', [(2, 5, 7, 64, 255), (1, 9, 9, 128, 75), (3, 4, 5, 32, 18)], ids=lambda s: 'x'.join(map(str, s)))
def test_head_fwd(shape, dt):
    """the implicit-GEMM kernel with a bias epilogue against float64 convolution + bias on the rounded operands (TOL of test_gpu_kernels.py)"""
    _lib, ops = api()
    B, H, W, Cin, N = shape
    g = torch.Generator().manual_seed(N)
    x = torch.randn(B, H, W, Cin, generator=g).to(dt)
    wgt = (torch.randn(N, Cin, 1, 1, generator=g) / Cin ** 0.5).to(dt)
    bias = torch.randn(N, generator=g)
    xh = torch.zeros(B, H + 2, W + 2, Cin, dtype=dt)
    xh[:, 1:-1, 1:-1] = x
    xd, bd = gpu(xh), gpu(bias)
    d = _lib.ConvDesc(ops._code(dt), B, H, W, Cin, N, 1, 1, 1, 1)
    wf, _ = ops.packed_weights(gpu(wgt.float()), d, dt, cache=False)
    out = nan_buf((B, H, W, N), FP)
    _lib.call('fva_head_fwd', C.byref(d), ops._p(xd), ops._p(wf), ops._p(bd), ops._p(out), ops._stream())
    want = x.double().reshape(-1, Cin) @ wgt.double().view(N, Cin).t() + bias.double()
    got = out.cpu().double().reshape(-1, N)
    assert torch.isfinite(got).all()
    err = ((got - want).abs().max() / want.abs().max()).item()
    assert err < TOL[key(dt)], err
    print(f'\n  fva_head_fwd {key(dt)} {shape}: max err / scale {err:.2e}')
