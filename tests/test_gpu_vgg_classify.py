"""The VGG classifiers on the device (classfication/models/vgg.py of the reference): the BatchNorm + ReLU passes element by element
against float64 (tests/streaming_measure.py), adaptive 7x7 pooling, the counter-based dropout, and whole train steps of the eight
factories against a stock-torch restatement on the CPU (tests/vgg_restatement.py) with the same weights.

The ReLU kink.  The backward passes decide dU = dz * (u > 0) from u = y * scale + shift recomputed in fp32; an element whose float64 u
is closer to zero than the fp32 limit of u itself may honestly land on either side.  Those elements are taken out of the element-wise
backward check, enter the limit of the sums with the whole magnitude of their term, and must be at most 0.1 % of the elements (the
seeded normal inputs below put none there: the count is printed by every case).

Every test prints its figures (pytest -s).
"""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import streaming_measure as sm
from vgg_restatement import NAMES, StockVGG, dropout_keep_mask, set_dropout

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
BF, FP = torch.bfloat16, torch.float32
NAN = float('nan')
KINK_SHARE_MAX = 1e-3


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def api():
    from fastvision_amd import _lib, ops
    return _lib, ops


def nan_buf(shape, dt):
    return torch.full(shape, NAN, dtype=dt, device=DEV)


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


def signed(g, n, lo, hi):
    return (torch.rand(n, generator=g) * (hi - lo) + lo) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)


def key(dt):
    return 'bf16' if dt == BF else 'f32'


# ================================================================================================ BatchNorm + ReLU passes
#  dt  B   H   W    C  pad  regime
RELU_CASES = [
    (BF, 2, 5, 7, 64, 1, 'C = 64 bf16, row_chunks 72 < 256, H*W = 35 not a multiple of anything'),
    (BF, 4, 56, 56, 128, 1, 'C = 128 bf16, the stage-2 map: 1.6 M elements, rounding bias'),
    (BF, 2, 14, 14, 512, 1, 'C = 512 bf16 (cpp 64), the stage-5 map: row_chunks 1024'),
    (FP, 2, 9, 13, 64, 1, 'C = 64 fp32, row_chunks 240, odd H and W'),
    (FP, 1, 3, 75, 128, 0, 'C = 128 fp32, row_chunks 2400 > 2048, no halo, B = 1'),
    (FP, 2, 7, 7, 512, 1, 'C = 512 fp32 (cpp 128), row_chunks 1152'),
]


def relu_inputs(dt, M, Cc, seed):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(M, Cc, generator=g) * 1.5 + 0.3).to(dt)
    dz = torch.randn(M, Cc, generator=g).to(dt)
    scale, shift = signed(g, Cc, 0.3, 2.0), torch.rand(Cc, generator=g) * 2 - 1
    mean, rstd = torch.randn(Cc, generator=g) * 0.5 + 0.3, torch.rand(Cc, generator=g) + 0.4
    gamma = signed(g, Cc, 0.5, 1.5)
    return y, dz, scale, shift, mean, rstd, gamma


def u_of(y, scale, shift, dt):
    return y.to(dt) * scale.to(dt) + shift.to(dt)


def near_kink(y, scale, shift):
    """Elements whose float64 u is closer to zero than the fp32 limit of u (factor 4): either side of the kink is honest."""
    u64, u32 = u_of(y, scale, shift, torch.float64), u_of(y, scale, shift, torch.float32)
    mag = torch.maximum((y.double() * scale.double()).abs(), shift.double().abs().expand_as(u64))
    return u64.abs() < sm.limit_of(u64, u32, mag)


def relu_terms(dz, y, scale, shift, mean, rstd, dt):
    yy = y.to(dt)
    du = dz.to(dt) * (u_of(y, scale, shift, torch.float64) > 0).to(dt)       # the mask is the float64 one in both precisions
    return du, du * (yy - mean.to(dt)) * rstd.to(dt)


def relu_bwd_apply(dz, y, scale, shift, mean, rstd, a, cb, cc, dt):
    yy = y.to(dt)
    du = dz.to(dt) * (u_of(y, scale, shift, torch.float64) > 0).to(dt)
    k1 = cb.to(dt) * rstd.to(dt)
    k2 = cc.to(dt) - k1 * mean.to(dt)
    t1, t2 = a.to(dt) * du, k1 * yy
    mag = torch.maximum(torch.maximum(t1.abs(), t2.abs()), k2.abs().expand_as(t1))
    return t1 + t2 + k2, mag


@pytest.mark.parametrize('case', RELU_CASES, ids=lambda c: '-'.join(str(v).replace('torch.', '') for v in c[:-1]))
def test_bn_relu_passes_against_float64(case):
    _lib, ops = api()
    lib = _lib.load()
    dt, B, H, W, Cc, pad, regime = case
    M, bf, code = B * H * W, dt == BF, ops._code(dt)
    y, dz, scale, shift, mean, rstd, gamma = relu_inputs(dt, M, Cc, 7 + W + Cc)
    kink = near_kink(y, scale, shift)
    share = kink.double().mean().item()
    assert share <= KINK_SHARE_MAX, f'{regime}: {share:.2e} of the elements sit on the kink'
    d = {k: v.to(DEV) for k, v in dict(y=y, dz=dz, scale=scale, shift=shift, mean=mean, rstd=rstd, gamma=gamma).items()}
    p = ops._p

    # ---- forward apply: continuous at the kink, so every element is checked
    zs = []
    for _ in range(2):
        z = nan_buf((B, H + 2 * pad, W + 2 * pad, Cc), dt)
        _lib.call('fva_bn_relu_apply', code, p(d['y']), p(d['scale']), p(d['shift']), p(z), pad, B, H, W, Cc, ops._stream())
        zs.append(z.cpu())
    assert torch.equal(bits(zs[0]), bits(zs[1])), 'apply: two runs differ'
    got = interior(zs[0], pad, regime).reshape(M, Cc)
    u64, u32 = u_of(y, scale, shift, torch.float64), u_of(y, scale, shift, torch.float32)
    mag = torch.maximum((y.double() * scale.double()).abs(), shift.double().abs().expand_as(u64))
    w_fwd = sm.check(got, u64.clamp_min(0), u32.clamp_min(0), mag, bf, bias=bf and got.numel() >= sm.BIAS_MIN_N, what=regime + ' apply')

    # ---- backward pass 1: the sums; an element on the kink may or may not be in them
    nb = lib.fva_bn_bwd_blocks(code, M, Cc)
    assert nb > 0
    n = -(-M // nb)
    t64 = relu_terms(dz, y, scale, shift, mean, rstd, torch.float64)
    t32 = relu_terms(dz, y, scale, shift, mean, rstd, torch.float32)
    raw = (dz.double(), dz.double() * (y.double() - mean.double()) * rstd.double())            # a term's size if its mask flips
    ref = torch.stack([t.sum(0) for t in t64])
    lim = torch.stack([sm.sum_limit(n, a.abs().sum(0), (b.double() - a).abs().sum(0)) + (r.abs() * kink).sum(0) for a, b, r in zip(t64, t32, raw)])
    parts = []
    for _ in range(2):
        part = nan_buf((lib.fva_bn_partial_rows(nb), 2, Cc), FP)
        _lib.call('fva_bn_relu_bwd_reduce', code, p(d['dz']), p(d['y']), p(d['scale']), p(d['shift']), p(d['mean']), p(d['rstd']), p(part), nb, M, Cc,
                  ops._stream())
        parts.append(part[:nb].cpu())
    assert torch.equal(parts[0], parts[1]), 'reduce: two runs differ'
    sums = parts[0].double().sum(0)
    w_sum = ((sums - ref).abs() / lim).max().item()
    assert torch.isfinite(sums).all() and w_sum <= 1.0, f'{regime}: sums worst err / limit {w_sum:.3f}'

    # ---- fva_bn_bwd_finalize (reused as is) on the kernel's own table, then pass 2
    rows = lib.fva_bn_partial_rows(nb)
    part = torch.zeros((rows, 2, Cc), dtype=FP, device=DEV)
    part[:nb] = parts[0].to(DEV)
    dgamma, dbeta, coef = nan_buf((Cc,), FP), nan_buf((Cc,), FP), nan_buf((3, Cc), FP)
    _lib.call('fva_bn_bwd_finalize', p(part), nb, rows, M, Cc, p(d['gamma']), p(d['rstd']), p(dgamma), p(dbeta), 0, p(coef), ops._stream())
    cf = coef.cpu()
    fin_lim = (nb + 2) * sm.EPS32 * parts[0].double().abs().sum(0)      # the finalize pass adds the nb rows in fp32 pairs, then in double
    assert ((dbeta.cpu().double() - sums[0]).abs() <= fin_lim[0]).all()
    assert ((dgamma.cpu().double() - sums[1]).abs() <= fin_lim[1]).all()
    dys = []
    for _ in range(2):
        dy = nan_buf((B, H + 2 * pad, W + 2 * pad, Cc), dt)
        _lib.call('fva_bn_relu_bwd_apply', code, p(d['dz']), p(d['y']), p(d['scale']), p(d['shift']), p(d['mean']), p(d['rstd']), p(coef), p(dy), pad,
                  B, H, W, Cc, ops._stream())
        dys.append(dy.cpu())
    assert torch.equal(bits(dys[0]), bits(dys[1])), 'bwd apply: two runs differ'
    got = interior(dys[0], pad, regime).reshape(M, Cc)
    r64, mag = relu_bwd_apply(dz, y, scale, shift, mean, rstd, cf[0], cf[1], cf[2], torch.float64)
    r32, _ = relu_bwd_apply(dz, y, scale, shift, mean, rstd, cf[0], cf[1], cf[2], torch.float32)
    keep = ~kink
    if kink.any():                       # an element on the kink: either side, i.e. with or without its a * dz term
        alt = r64 + cf[0].double() * dz.double() * torch.where(u64 > 0, -1.0, 1.0)
        on = got.double()[kink]
        lo, hi = torch.minimum(r64[kink], alt[kink]), torch.maximum(r64[kink], alt[kink])
        slack = 0.5 * sm.bf16_ulp(hi.abs().maximum(lo.abs())) + 1e-5 * mag[kink]
        assert ((on >= lo - slack) & (on <= hi + slack)).all(), 'an element on the kink is on neither side'
    w_bwd = sm.check(got[keep], r64[keep], r32[keep], mag[keep], bf, bias=bf and int(keep.sum()) >= sm.BIAS_MIN_N, what=regime + ' bwd apply')
    print(f'\n  bn_relu {key(dt)} [{regime}]: worst err / limit apply {w_fwd:.3f}, sums {w_sum:.3f}, bwd apply {w_bwd:.3f}; '
          f'on the kink (excluded) {int(kink.sum())} of {kink.numel()} = {share:.2e}')


def test_bn_bias_helpers_against_float64():
    _lib, ops = api()
    g = torch.Generator().manual_seed(3)
    Cc = 512
    gamma, beta, rm = signed(g, Cc, 0.5, 1.5), torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    rv, b = torch.rand(Cc, generator=g) + 0.1, torch.randn(Cc, generator=g)
    d = [t.to(DEV) for t in (gamma, beta, rm, rv, b)]
    scale, shift = nan_buf((Cc,), FP), nan_buf((Cc,), FP)
    _lib.call('fva_bn_eval_coeffs_bias', Cc, *[ops._p(t) for t in d], 1e-5, ops._p(scale), ops._p(shift), ops._stream())
    s64 = gamma.double() / (rv.double() + 1e-5).sqrt()
    h64 = beta.double() + (b.double() - rm.double()) * s64
    assert ((scale.cpu().double() - s64).abs() <= 4 * sm.EPS32 * s64.abs()).all()
    hm = torch.maximum(beta.double().abs(), ((b.double() - rm.double()) * s64).abs())
    assert ((shift.cpu().double() - h64).abs() <= 8 * sm.EPS32 * hm).all()
    rmd = rm.to(DEV)
    _lib.call('fva_bn_bias_running_mean', Cc, ops._p(rmd), ops._p(d[4]), 0.1, ops._stream())
    want = rm.double() + 0.1 * b.double()
    assert ((rmd.cpu().double() - want).abs() <= 4 * sm.EPS32 * (rm.double().abs() + 0.1 * b.double().abs())).all()


# ================================================================================================ adaptive 7x7 pooling
POOL_HW = [(7, 7), (8, 8), (10, 10), (14, 14), (3, 3), (1, 1), (7, 10)]


@pytest.mark.parametrize('hw,Cc,dtype', list(itertools.product(POOL_HW, [512, 64], [FP, BF])))
def test_adaptive_avg_pool7_forward_backward_against_float64(hw, Cc, dtype):
    """Tolerances of test_gpu_classify.py's global-average-pool test: forward 1e-5 of the scale, backward 1e-6 (fp32) / 8e-3 (bf16: dx is
    stored in bf16).  The output of THIS pooling is in the compute dtype (the first Linear's operand as stored), so a bf16 output gets the
    half bf16 ulp of its one store on top of the 1e-5."""
    from fastvision_amd import ops, vgg_ops
    H, W = hw
    B = 2
    gen = torch.Generator().manual_seed(Cc + 10 * H + W)
    x = torch.randn(B, Cc, H, W, generator=gen).to(dtype)
    g = torch.randn(B, Cc * 49, generator=gen).to(dtype)
    x64 = x.double().requires_grad_(True)
    want = torch.flatten(F.adaptive_avg_pool2d(x64, (7, 7)), 1)
    want.backward(g.double())
    want, want_dx = want.detach(), x64.grad
    for form in ('halo', 'nchw'):
        if form == 'halo':
            buf, view = ops.halo_alloc(B, Cc, H, W, dtype, DEV, 1)
            buf.fill_(NAN)                                              # a kernel that reads one pixel off the interior shows it
            view.copy_(x.to(DEV))
            buf.requires_grad_(True)
            xin = buf[:, 1:1 + H, 1:1 + W, :].permute(0, 3, 1, 2)
            assert ops.halo_info(xin.detach(), dtype) is not None
        else:
            leaf = x.float().contiguous().to(DEV).requires_grad_(True)
            xin = leaf
        runs = []
        for _ in range(2):
            if form == 'halo':
                buf.grad = None
            else:
                leaf.grad = None
            out = vgg_ops.adaptive_avg_pool7_flatten(xin, dtype)
            out.backward(g.to(DEV))
            dx = buf.grad[:, 1:1 + H, 1:1 + W, :].permute(0, 3, 1, 2) if form == 'halo' else leaf.grad
            runs.append((out.detach().clone().cpu(), dx.detach().clone().cpu()))
        (o1, d1), (o2, d2) = runs
        assert o1.dtype == dtype and tuple(o1.shape) == (B, Cc * 49)
        assert torch.equal(bits(o1), bits(o2)) and torch.equal(d1, d2), form
        lim = 1e-5 * want.abs().max() + (0.5 * sm.bf16_ulp(want) if dtype == BF else 0.0)
        assert ((o1.double() - want).abs() <= lim).all(), (form, rel_err(o1, want))
        tol = 1e-6 if dtype == FP else 8e-3
        assert rel_err(d1, want_dx) < tol, (form, rel_err(d1, want_dx))
        if form == 'halo':
            border = buf.grad.clone()
            border[:, 1:1 + H, 1:1 + W, :] = 0
            assert not border.any()


# ================================================================================================ dropout
def _sigma(q, n):
    return math.sqrt(q * (1 - q) / n)


@pytest.mark.parametrize('p,dtype', list(itertools.product([0.5, 0.2], [BF, FP])))
def test_dropout_mask_statistics_values_and_backward(p, dtype):
    from fastvision_amd import fc_ops
    R, N = 32, 4096
    n = R * N
    gen = torch.Generator().manual_seed(17)
    x = (torch.randn(R, N, generator=gen).abs() + 0.1).to(dtype)
    g = torch.randn(R, N, generator=gen).to(dtype)
    drop = nn.Dropout(p).train()
    scale = 1.0 / (1.0 - p)

    def run(seed):
        state = fc_ops.new_dropout_state(seed).to(DEV)
        xd = x.to(DEV).requires_grad_(True)
        o1 = fc_ops.dropout(xd, drop, state, dtype)
        o1.backward(g.to(DEV))
        o2 = fc_ops.dropout(x.to(DEV), drop, state, dtype)             # the next call (the model's second Dropout layer shares the state)
        torch.cuda.synchronize()
        return o1.detach().cpu(), o2.detach().cpu(), xd.grad.cpu(), state.cpu().tolist()

    o1, o2, dx, st = run(1234)
    assert st == [1234, 2, 0, 0], st                                   # two calls advanced the counter on the device, the block count is back at 0
    m1, m2 = o1 != 0, o2 != 0
    want = (x.double() * scale).to(dtype)
    assert torch.equal(bits(o1), bits(torch.where(m1, want, torch.zeros_like(want)))), 'kept = x / (1 - p) rounded once, dropped = 0'
    assert torch.equal(bits(o2), bits(torch.where(m2, want, torch.zeros_like(want))))
    wdx = torch.where(m1, (g.double() * scale).to(dtype), torch.zeros_like(g))
    assert torch.equal(bits(dx), bits(wdx)), 'backward = dout * mask / (1 - p)'
    msg = []
    for name, m in (('call 1', m1), ('call 2', m2)):
        rate = m.double().mean().item()
        msg.append(f'{name} keep {rate:.4f}')
        assert abs(rate - (1 - p)) <= 5 * _sigma(p, n), (name, rate)
    q = p * p + (1 - p) * (1 - p)
    agree = (m1 == m2).double().mean().item()
    msg.append(f'calls agree {agree:.4f}')
    assert abs(agree - q) <= 5 * _sigma(q, n), agree
    f1 = m1.flatten()
    for s in (1, 64, 4096):
        a = (f1[:-s] == f1[s:]).double().mean().item()
        msg.append(f'shift {s} {a:.4f}')
        assert abs(a - q) <= 5 * _sigma(q, n - s), (s, a)
    o1b, o2b, dxb, _ = run(1234)
    assert torch.equal(bits(o1), bits(o1b)) and torch.equal(bits(o2), bits(o2b)) and torch.equal(bits(dx), bits(dxb)), 'same seed, same masks'
    o1c, _, _, _ = run(1235)
    other = ((o1c != 0) == m1).double().mean().item()
    assert abs(other - q) <= 5 * _sigma(q, n), other
    print(f'\n  dropout p={p} {key(dtype)}: ' + ', '.join(msg) + f', other seed agrees {other:.4f} (q = {q:.4f} +- {5 * _sigma(q, n):.4f})')


@pytest.mark.parametrize('seed,counter,p', [(0, 0, 0.5), (1234, 0, 0.5), (0x1234567887654321, 0x100000003, 0.2), (3, 7, 0.9)])
def test_dropout_mask_is_philox4x32_10(seed, counter, p):
    """The device's mask, element by element, against the host restatement of the ten rounds (tests/vgg_restatement.py, pinned to the
    published known-answer vectors by tests/test_vgg_cpu.py): the generator and its keying (seed, call counter, element index) are the
    ones the header names."""
    from fastvision_amd import fc_ops
    n = 32 * 4096
    x = torch.ones(32, 4096, device=DEV)
    state = torch.tensor([seed, counter, 0, 0], dtype=torch.int64, device=DEV)
    out = fc_ops.dropout(x, nn.Dropout(p).train(), state, FP)
    want = dropout_keep_mask(seed, counter, n, p).view(32, 4096)
    assert torch.equal((out != 0).cpu(), want)
    assert state.cpu().tolist() == [seed, counter + 1, 0, 0]


def test_dropout_mask_does_not_depend_on_the_dtype():
    from fastvision_amd import fc_ops
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(32, 4096, generator=gen).abs() + 0.1
    drop = nn.Dropout(0.5).train()
    masks = []
    for dt in (BF, FP):
        state = fc_ops.new_dropout_state(99).to(DEV)
        masks.append((fc_ops.dropout(x.to(dt).to(DEV), drop, state, dt) != 0).cpu())
    assert torch.equal(masks[0], masks[1])


def test_dropout_on_relu_output_with_zeros():
    from fastvision_amd import fc_ops
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(32, 4096, generator=gen).clamp_min(0).to(BF)
    out = fc_ops.dropout(x.to(DEV), nn.Dropout(0.5).train(), fc_ops.new_dropout_state(5).to(DEV), BF).cpu()
    dbl = (x.double() * 2).to(BF)
    assert ((out == 0) | (bits(out) == bits(dbl))).all() and not out[x == 0].any()


def test_dropout_eval_and_p0_launch_nothing(monkeypatch):
    from fastvision_amd import _lib, fc_ops
    x = torch.randn(8, 4096, device=DEV).abs()
    state = fc_ops.new_dropout_state(1).to(DEV)
    torch.cuda.synchronize()
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    torch.cuda.set_sync_debug_mode('error')
    try:
        assert fc_ops.dropout(x, nn.Dropout(0.5).eval(), state) is x
        assert fc_ops.dropout(x, nn.Dropout(0.0).train(), state) is x
        drop = nn.Dropout(0.5).train()
        drop.p = 0.0                                                  # read at call time
        assert fc_ops.dropout(x, drop, state) is x
        assert calls == []
        drop.p = 0.5
        y = fc_ops.dropout(x, drop, state, FP)
        assert calls == ['fva_dropout_fwd']
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert state.cpu().tolist() == [1, 1, 0, 0] and y is not x


# ================================================================================================ whole models against the CPU restatement
def _pair(name, seed, num_classes=10, p=0.0):
    from fastvision_amd.classfication import models
    torch.manual_seed(seed)
    ref = StockVGG(name, num_classes=num_classes)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, nn.BatchNorm2d):                         # not the identity: a BatchNorm whose affine and statistics matter
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
            if isinstance(m, nn.Conv2d):
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                if not name.endswith('_bn'):
                    # torch's default init lets the signal die out through 13 ReLU layers without BatchNorm: the first layers' weight
                    # gradients then cancel so badly that the fp32 CPU restatement itself is 1.7e-2 (vgg16, 224^2, vgg1.0.weight) from
                    # its own float64 run.  He initialisation (fan_out, as torchvision's VGG) keeps every layer at unit scale.
                    m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / (m.out_channels * 9)))
    net = getattr(models, name)(num_classes=num_classes)
    net.load_state_dict(ref.state_dict(), strict=True)
    set_dropout(ref, p)
    set_dropout(net, p)
    return ref.train(), net.to(DEV).train()


def _batch(B, S, seed, num_classes=10):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, S, S, generator=gen), torch.randint(0, num_classes, (B,), generator=gen)


def _windows(x):
    """[B, C, H, W] -> [B, C, H/2, W/2, 4]: the 2x2 windows of MaxPool2d(2, 2) in scan order"""
    B, Cc, H, W = x.shape
    return x.reshape(B, Cc, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, Cc, H // 2, W // 2, 4)


def _first_max(xw):
    """index of the first maximum of each window (torch's and the kernel's choice among equals)"""
    idx = torch.arange(4, device=xw.device).expand_as(xw)
    return torch.where(xw == xw.max(-1, keepdim=True).values, idx, torch.full_like(idx, 4)).min(-1).values


def _device_masks(name, net, images, dtype):
    """What the device decides at the two discontinuities of the network: (z > 0) of every convolution block and the arg-max of every
    pooling window, from a twin of the model (the statistics of ``net`` stay untouched; the kernels are deterministic, so the twin's forward
    pass is the real step's bit for bit)."""
    import fastvision_amd
    from fastvision_amd import vgg_ops
    from fastvision_amd.classfication import models
    twin = getattr(models, name)(num_classes=10)
    twin.load_state_dict(net.state_dict(), strict=True)
    twin = twin.to(DEV).train()
    masks, args, x = [], [], images.to(DEV)
    with torch.no_grad(), fastvision_amd.compute_dtype(dtype):
        for s in range(1, 6):
            seq = list(getattr(twin, f'vgg{s}'))
            for i, m in enumerate(seq):
                if isinstance(m, nn.Conv2d):
                    x = vgg_ops.conv_bn_relu(x, m, seq[i + 1]) if isinstance(seq[i + 1], nn.BatchNorm2d) else vgg_ops.conv_bias_relu(x, m)
                    masks.append((x > 0).cpu())
            args.append(_first_max(_windows(x.contiguous())).cpu())
            x = vgg_ops.max_pool2(x)
    return masks, args


def _ref64_forward(r64, images, decisions):
    """The restatement in float64.  ReLU and max pooling are discontinuous in their gradients: an element whose float64 pre-activation u is
    closer to zero than ANY fp32 evaluation of it can resolve may honestly be masked either way, two window elements closer to each other
    than that may honestly swap, and in a layer of M rows ONE such decision moves a weight gradient by ~1 / sqrt(M) of its scale
    (measured: vgg11_bn at 64^2, one element of vgg4.0's 65536 on the other side, vgg4.0.weight 7.9e-2 off, everything upstream 5e-3,
    everything else 4e-6).  So the reference takes the device's side on exactly the decisions it certifies itself as undecidable in fp32:
    |u64| <= lim (ReLU), |a - b| <= lim_a + lim_b (pooling), lim = 2 K 2^-24 * (sum |w||x| + |b|, through the BatchNorm affine), K = 9 Cin
    + 4 the length of the fp32 chain behind u -- the rule of the element-wise tests above -- and they must be at most 0.1 % of a layer.
    Returns (logits, largest share)."""
    masks, args = decisions
    x, it, worst = images.double(), iter(masks), 0.0
    for s in range(1, 6):
        seq = list(getattr(r64, f'vgg{s}'))
        for i, m in enumerate(seq):
            if not isinstance(m, nn.Conv2d):
                continue
            bn = seq[i + 1] if isinstance(seq[i + 1], nn.BatchNorm2d) else None
            y = m(x)
            u = bn(y) if bn is not None else y
            with torch.no_grad():
                mag = F.conv2d(x.abs(), m.weight.abs(), m.bias.abs(), 1, 1)
                if bn is not None:
                    sc = (bn.weight / (y.var((0, 2, 3), unbiased=False) + bn.eps).sqrt()).abs()[None, :, None, None]
                    mag = (mag + mag.mean((0, 2, 3), keepdim=True)) * sc + bn.bias.abs()[None, :, None, None]
                lim = 2 * (9 * m.in_channels + 4) * sm.EPS32 * mag
                own, dev = u > 0, next(it)
                mism = own != dev
                assert (u.abs()[mism] <= lim[mism]).all(), f'vgg{s}.{i}: the device masks an element that is not on the kink'
                worst = max(worst, mism.double().mean().item())
                keep = torch.where(mism, dev, own).double()
            x = u * keep
        zw = _windows(x)
        with torch.no_grad():
            lw = _windows(lim)
            own, dev = _first_max(zw), args[s - 1]
            mism = own != dev
            gap = zw.max(-1).values - zw.gather(-1, dev[..., None])[..., 0]
            room = lw.gather(-1, own[..., None])[..., 0] + lw.gather(-1, dev[..., None])[..., 0]
            assert (gap[mism] <= room[mism]).all(), f'pool{s}: the device picks an element that is not a maximum'
            worst = max(worst, mism.double().mean().item())
            pick = torch.where(mism, dev, own)
        x = zw.gather(-1, pick[..., None])[..., 0]
    assert worst <= KINK_SHARE_MAX, worst
    return r64.classifier(torch.flatten(r64.gmp(x), 1)), worst


def _both_steps(name, S, dtype, seed=5, adopt=True):
    """One train step on the device and in the float64 restatement (same weights).  Returns (ref, r64, net, ...): ``ref`` is the fp32
    restatement with the weights (for the eval-mode comparison), ``r64`` carries the reference gradients and statistics."""
    import fastvision_amd
    from fastvision_amd.loss import CrossEntropyLoss
    ref, net = _pair(name, seed)
    images, labels = _batch(2, S, seed + 2)
    masks = _device_masks(name, net, images, dtype) if adopt else None
    r64 = StockVGG(name, num_classes=10).double()
    r64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in ref.state_dict().items()})
    set_dropout(r64, 0.0)
    r64.train()
    plain = None
    if adopt:                # the restatement's own decisions: logits and loss are continuous in them, so they are compared as they are
        import copy
        with torch.no_grad():
            pl = copy.deepcopy(r64)(images.double())
            plain = (pl, F.cross_entropy(pl, labels).item())
    rl, share = _ref64_forward(r64, images, masks) if adopt else (r64(images.double()), 0.0)
    rloss = F.cross_entropy(rl, labels)
    rloss.backward()
    with fastvision_amd.compute_dtype(dtype):
        gl = net(images.to(DEV))
        gloss = CrossEntropyLoss()(gl, labels.to(DEV))
        gloss.backward()
    torch.cuda.synchronize()
    assert gl.dtype == torch.float32 and tuple(gl.shape) == (2, 10)
    print(f'\n  {name} {key(dtype)} {S}: fp32 largest share of a layer\'s decisions taken from the device {share:.1e}')
    _both_steps.plain, _both_steps.share = plain, share
    return ref, r64, net, rl.detach(), rloss.item(), gl.detach().cpu(), gloss.item(), images


def _grad_names(name):
    names = ['vgg1.0.weight', 'vgg3.0.weight', 'classifier.0.weight', 'classifier.6.bias']
    return names + (['vgg2.1.weight'] if name.endswith('_bn') else [])


def _check_fp32(name, S):
    import fastvision_amd
    ref, r64, net, rl, rloss, gl, gloss, images = _both_steps(name, S, FP)
    rp, gp = dict(r64.named_parameters()), dict(net.named_parameters())
    figs = {'logits': rel_err(gl, rl), 'loss': abs(gloss - rloss) / abs(rloss)}
    pl, ploss = _both_steps.plain                             # without anything taken from the device
    figs['logits (plain restatement)'], figs['loss (plain restatement)'] = rel_err(gl, pl), abs(gloss - ploss) / abs(ploss)
    for k in _grad_names(name):
        figs[k] = rel_err(gp[k].grad, rp[k].grad)
    if name.endswith('_bn'):
        rb, gb = dict(r64.named_buffers()), dict(net.named_buffers())
        for k, v in rb.items():
            if k.endswith('num_batches_tracked'):
                assert gb[k].item() == v.item() == 1, k
            else:
                figs[k] = rel_err(gb[k], v)
        # the convolution bias in front of BatchNorm: its gradient is rounding noise (the reference itself: <= 2e-5 of the layer's
        # max |bn.bias.grad|); exact zeros are fine, 1e-4 of that is the bar
        for stage in range(1, 6):
            seq = getattr(net, f'vgg{stage}')
            for i, m in enumerate(seq):
                if isinstance(m, nn.Conv2d):
                    gb_ = m.bias.grad
                    assert gb_ is not None and gb_.dtype == torch.float32 and gb_.shape == m.bias.shape
                    assert gb_.abs().max().item() <= 1e-4 * seq[i + 1].bias.grad.abs().max().item(), (stage, i)
    worst = max(figs, key=figs.get)
    print(f'\n  {name} fp32 {S}x{S}: logits {figs["logits"]:.2e} loss {figs["loss"]:.2e}; worst {worst} {figs[worst]:.2e}')
    assert all(np.isfinite(v) and v < 1e-3 for v in figs.values()), {k: v for k, v in figs.items() if not v < 1e-3}
    # eval mode on the same weights and statistics: running statistics and the convolution bias folded into the affine
    net.load_state_dict(ref.state_dict(), strict=True)
    ref.eval(), net.eval()
    with torch.no_grad(), fastvision_amd.compute_dtype(FP):
        e = rel_err(net(images.to(DEV)), ref(images))
    print(f'  {name} fp32 {S}x{S} eval logits {e:.2e}')
    assert e < 1e-3, e


@pytest.mark.parametrize('name', NAMES)
def test_train_step_fp32_64px_all_factories(name):
    _check_fp32(name, 64)


@pytest.mark.parametrize('name,S', [('vgg11_bn', 224), ('vgg16', 224), ('vgg16_bn', 256)])
def test_train_step_fp32_full_size(name, S):
    _check_fp32(name, S)


class _Store(torch.autograd.Function):
    """a bf16 store: the value is rounded on the way forward, its gradient on the way back"""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().float()

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().float()


def _emulated_bf16_step(ref, images, labels):
    """The fp32 restatement with a bf16 rounding at every point where the kernels store (the r() emulation of tests/test_gpu_vgg.py): the
    image batch, the packed weights (values only: their gradients stay fp32), every convolution output, every activation, the pooled
    vector, the hidden layers of the classifier, and the gradient of each of these on the way back.  Leaves the gradients in ``ref``."""
    r = _Store.apply
    rw = lambda w: w + (w.bfloat16().float() - w).detach()
    ref.zero_grad(set_to_none=True)
    x = r(images)
    for s in range(1, 6):
        seq = list(getattr(ref, f'vgg{s}'))
        for i, m in enumerate(seq):
            if not isinstance(m, nn.Conv2d):
                continue
            if isinstance(seq[i + 1], nn.BatchNorm2d):
                y = r(F.conv2d(x, rw(m.weight), None, 1, 1))
                x = r(F.relu(seq[i + 1](y + m.bias[None, :, None, None])))
            else:
                x = r(F.relu(F.conv2d(x, rw(m.weight), m.bias, 1, 1)))
        x = ref.maxpool(x)
    x = r(torch.flatten(ref.gmp(x), 1))
    c = ref.classifier
    x = r(F.relu(F.linear(x, rw(c[0].weight), c[0].bias)))
    x = r(F.relu(F.linear(x, rw(c[3].weight), c[3].bias)))
    F.cross_entropy(F.linear(x, rw(c[6].weight), c[6].bias), labels).backward()


def _cosine(a, b):
    a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
    return (a @ b / (a.norm() * b.norm()).clamp_min(1e-300)).item()


# measured cosine of the bf16 store emulation with the float64 restatement (CPU, seed 5, 2 x 3 x 224^2) and the bar 1 - 2 (1 - cosine) from it
BF16_COSINE = {
    'vgg16_bn': {'vgg1.0.weight': (0.7917, 0.58), 'vgg3.0.weight': (0.7942, 0.58), 'classifier.0.weight': (0.9458, 0.89),
                 'classifier.6.bias': (1.0, 0.96), 'vgg2.1.weight': (0.7526, 0.50)},
    'vgg16': {'vgg1.0.weight': (0.9067, 0.81), 'vgg3.0.weight': (0.9458, 0.89), 'classifier.0.weight': (0.9942, 0.96), 'classifier.6.bias': (1.0, 0.96)},
}


@pytest.mark.parametrize('name', ['vgg16_bn', 'vgg16'])
def test_train_step_bf16_224(name):
    """The bars of test_gpu_fullsize.py (set on Darknet-53): outputs within 1.3e-1 of their scale, gradient norms within 1.2e-1, cosine
    of the sampled gradients above 0.96.  Gradient norms: all parameters except the convolution biases in front of a BatchNorm (zero).
    Outputs and norms hold on VGG as they stand (measured: vgg16_bn 8.1e-2 / 1.19e-1, vgg16 1.0e-2 / 1.07e-1).  The cosine does not
    (measured on the device: vgg16_bn 0.781 at vgg2.1.weight, vgg16 0.898 at vgg1.0.weight): two images give a layer of VGG few rows, and
    every ReLU / pooling decision that bf16 rounding flips moves a gradient by ~1 / sqrt(rows).  Not widened by eye: the CPU restatement
    with a bf16 rounding wherever the kernels store (_emulated_bf16_step) was run on these weights and this batch, ITS distance
    d = 1 - cosine from the float64 restatement taken per tensor, and the bar is 1 - 2 d (the kernels also reorder sums) where that is
    below the original 0.96, rounded down to two digits and FIXED here (BF16_COSINE: emulation cosine -> bar; the emulation is run again
    and printed, it does not move the bar)."""
    ref, r64, net, rl, rloss, gl, gloss, images = _both_steps(name, 224, BF, adopt=False)       # the plain float64 restatement: bf16 is not a kink matter
    rp, gp = dict(r64.named_parameters()), dict(net.named_parameters())
    _emulated_bf16_step(ref.train(), images, _batch(2, 224, 7)[1])
    ep = dict(ref.named_parameters())
    herr = rel_err(gl, rl)
    rel, cos, bar = {}, {}, {}
    skip = {f'{n}.bias' for n, m in ref.named_modules() if isinstance(m, nn.Conv2d)} if name.endswith('_bn') else set()
    for k, p in rp.items():
        if k in skip:
            continue
        a, b = gp[k].grad.double().cpu(), p.grad.double()
        assert torch.isfinite(a).all(), k
        rel[k] = abs(a.norm().item() - b.norm().item()) / max(b.norm().item(), 1e-300)
    for k in _grad_names(name):
        cos[k] = _cosine(gp[k].grad, rp[k].grad)
        bar[k] = (BF16_COSINE[name][k][1], _cosine(ep[k].grad, rp[k].grad))
    wk = max(rel, key=rel.get)
    print(f'\n  {name} bf16 224: logits {herr:.2e} of scale, loss {gloss:.5f} vs {rloss:.5f}, gradient norms median {np.median(list(rel.values())):.2e} '
          f'max {rel[wk]:.2e} ({wk}); cosine device / emulation / bar: ' + ', '.join(f'{k} {cos[k]:.4f} / {bar[k][1]:.4f} / {bar[k][0]:.2f}' for k in cos))
    assert herr < 1.3e-1
    assert rel[wk] < 1.2e-1, wk
    for k in cos:
        assert cos[k] > bar[k][0], (k, cos[k], bar[k])


# ================================================================================================ the train step as a whole
def _train_parts(name='vgg11_bn', seed=3, p=0.5):
    from fastvision_amd import FusedSGD
    from fastvision_amd.classfication import models
    from fastvision_amd.loss import CrossEntropyLoss
    torch.manual_seed(seed)
    net = getattr(models, name)(num_classes=10)
    set_dropout(net, p)
    net = net.to(DEV).train()
    opt = FusedSGD(net.parameters(), lr=0.01, momentum=0.9, nesterov=True, weight_decay=5e-4, capturable=True)
    return net, CrossEntropyLoss(), opt


def _step(net, crit, opt, images, labels):
    pred = net(images)
    opt.zero_grad(set_to_none=True)
    loss = crit(pred, labels)
    loss.backward()
    opt.step()
    return loss.detach().clone()


def test_train_step_runs_without_aten_compute(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('ATen op in the VGG train step')
    net, crit, opt = _train_parts('vgg16_bn')
    images, labels = _batch(2, 64, 1)
    for name in ('dropout', 'adaptive_avg_pool2d', 'batch_norm', 'relu', 'linear', 'max_pool2d'):
        monkeypatch.setattr(F, name, refuse)
    loss = _step(net, crit, opt, images.to(DEV), labels.to(DEV))
    monkeypatch.undo()
    assert torch.isfinite(loss).item()
    assert net._dropout_state.cpu().tolist()[1:] == [2, 0, 0]


def test_train_step_and_accuracy_do_not_synchronise_the_host():
    from fastvision_amd.metrics import Accuracy
    net, crit, opt = _train_parts('vgg11_bn')
    images, labels = _batch(4, 64, 2)
    images, labels = images.to(DEV), labels.to(DEV)
    acc = Accuracy()
    _step(net, crit, opt, images, labels)
    acc(net(images).detach(), labels)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        pred = net(images)
        opt.zero_grad(set_to_none=True)
        loss = crit(pred, labels)
        loss.backward()
        opt.step()
        a = acc(pred.detach(), labels)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item() and 0.0 <= a.item() <= 1.0


def test_graphed_step_with_dropout_is_bit_identical_with_eager():
    """Dropout at 0.5: the replayed graph can only follow the eager run if seed and call counter live on the device, the kernel advances
    the counter itself, and the warm-up / capture steps are rolled back with the other buffers."""
    from fastvision_amd import ops
    from fastvision_amd.graphs import GraphedTrainStep
    gen = torch.Generator().manual_seed(5)
    batches = [(torch.randn(4, 3, 64, 64, generator=gen), torch.randint(0, 10, (4, 1), generator=gen).float()) for _ in range(3)]
    prev = ops.set_wgrad_side_stream(False)
    try:
        net, crit, opt = _train_parts()
        want = [_step(net, crit, opt, im.to(DEV), lab.to(DEV)) for im, lab in batches]
        torch.cuda.synchronize()
    finally:
        ops.set_wgrad_side_stream(prev)
    net2, crit2, opt2 = _train_parts()
    step = GraphedTrainStep(net2, lambda p, t: crit2(p, t), opt2, batches[0][0].to(DEV), batches[0][1].to(DEV))
    assert net2._dropout_state.cpu().tolist() == [3, 0, 0, 0]          # warm-up and capture rolled back
    got = [step(im.to(DEV), lab.to(DEV)).clone() for im, lab in batches]
    torch.cuda.synchronize()
    assert len({w.item() for w in want}) == 3
    for a, b in zip(got, want):
        assert torch.equal(a, b), (a, b)
    assert net._dropout_state.cpu().tolist() == net2._dropout_state.cpu().tolist() == [3, 6, 0, 0]
    for (k, p), q in zip(net.state_dict().items(), net2.state_dict().values()):
        assert torch.equal(p, q), k
    for p, q in zip(net.parameters(), net2.parameters()):
        assert torch.equal(opt.state[p]['momentum_buffer'], opt2.state[q]['momentum_buffer'])


def test_same_seed_trains_to_the_same_bits_and_dropout_matters():
    from fastvision_amd import ops
    images, labels = _batch(4, 64, 9)
    prev = ops.set_wgrad_side_stream(False)
    try:
        losses = []
        for seed, p in ((3, 0.5), (3, 0.5), (3, 0.0)):
            net, crit, opt = _train_parts(seed=seed, p=p)
            losses.append([_step(net, crit, opt, images.to(DEV), labels.to(DEV)).item() for _ in range(2)])
    finally:
        ops.set_wgrad_side_stream(prev)
    assert losses[0] == losses[1] and losses[0] != losses[2], losses


def test_fit_trains_vgg11_bn_with_dropout():
    from fastvision_amd import FusedSGD
    from fastvision_amd.classfication.models import vgg11_bn
    from fastvision_amd.loss import CrossEntropyLoss
    from fastvision_amd.utils import Fit
    gen = torch.Generator().manual_seed(11)
    labels = torch.arange(16) % 4
    images = torch.randn(16, 3, 64, 64, generator=gen) * 0.5
    for i in range(16):                                     # a learnable set: the class shows in the colour
        images[i, labels[i] % 3] += 1.0 + float(labels[i] // 3)
    torch.manual_seed(0)
    net = vgg11_bn(num_classes=10).to(DEV)
    assert net.classifier[2].p == 0.5
    opt = FusedSGD(net.parameters(), lr=0.01, momentum=0.9, nesterov=True, weight_decay=5e-4)
    fit = Fit(net, torch.device(DEV), opt, None, CrossEntropyLoss(), end_epoch=20, train_loader=[(images, labels)], save_last=None)
    fit.run_epoches()
    losses = [h[0] for h in fit.history]
    print('fit losses', [round(l, 4) for l in losses])
    assert len(losses) == 20 and np.isfinite(losses).all()
    assert losses[-1] < 0.5 * losses[0], losses
