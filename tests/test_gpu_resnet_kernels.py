"""The streaming kernels of csrc/resnet.hip element by element against the float64 restatement (tests/resnet_restatement.py), computed from
exactly the operands the kernel reads (bf16 inputs are made on the host, rounded once, and that tensor is both uploaded and fed to the
reference).  The measure is tests/streaming_measure.py, the rule of tests/test_gpu_streaming.py: bf16 outputs within half a bf16 ulp of
the float64 value (plus the fp32 limit) and unbiased; fp32 outputs within 4 x (the error of a plain fp32 torch evaluation + 2^-24 of the
largest term); sums by the (n + 2) * 2^-24 * sum|term| rule; copies and selections (patches, pooling, subsample, dr) bit for bit; halo
borders +0 bit for bit in outputs allocated full of NaN.  Every launch runs twice and must give the same bits.

Launch geometry the shapes are chosen by (csrc/resnet.hip): the BatchNorm + add + ReLU kernels run 256 threads as ncol = min(cpp, 256)
chunk columns x rpi = 256 / ncol pixels, cpp = C / 8 (bf16) or C / 4 (fp32); fp32 at C = 2048 (cpp 512) takes two column passes.  The
backward reduce gives a block max(ceil(M / 2048), 8 * rpi) pixel rows.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import resnet_restatement as rr
import streaming_measure as sm

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float32
DEV = 'cuda:0'
NAN = float('nan')
TOL = {'f32': 1e-4, 'bf16': 1e-2}          # tests/test_gpu_kernels.py: the implicit-GEMM tolerance
KINK_SHARE_MAX = 1e-3                      # tests/test_gpu_vgg_classify.py


def api():
    from fastvision_amd import _lib, ops
    return _lib, ops


def key(dt):
    return 'bf16' if dt == BF else 'f32'


def nan_buf(shape, dt):
    return torch.full(shape, NAN, dtype=dt, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def interior(buf, pad, what='', nan_ok=False):
    """A downloaded halo output: nothing is NaN, the border is +0 bit for bit; returns the interior."""
    assert nan_ok or not torch.isnan(buf).any(), f'{what}: NaN left in the output'
    if pad == 0:
        return buf
    Hp, Wp = buf.shape[1], buf.shape[2]
    border = torch.ones(Hp, Wp, dtype=torch.bool)
    border[pad:Hp - pad, pad:Wp - pad] = False
    assert not bits(buf)[:, border].any(), f'{what}: the border is not +0'
    return buf[:, pad:Hp - pad, pad:Wp - pad]


def in_halo(t, pad, fill=NAN):
    """An INPUT halo buffer around the dense NHWC tensor t; a NaN border shows a kernel that reads one pixel off."""
    if pad == 0:
        return t.contiguous()
    B, H, W, Cc = t.shape
    buf = torch.full((B, H + 2 * pad, W + 2 * pad, Cc), fill, dtype=t.dtype)
    buf[:, pad:pad + H, pad:pad + W] = t
    return buf


def signed(g, n, lo, hi):
    return (torch.rand(n, generator=g) * (hi - lo) + lo) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def twice(launch):
    """Run a launch twice into fresh NaN buffers; the outputs (tuples of CPU tensors) must agree bit for bit.  Returns the first."""
    a, b = launch(), launch()
    for x, y in zip(a, b):
        assert same_bits(x, y), 'two runs differ'
    return a


# ================================================================================================ the stem's patch matrix
PATCH_CASES = [(2, 3, 32, 32), (1, 3, 14, 18), (1, 1, 8, 8), (1, 4, 16, 16)]       # non-square with OW odd; Kp 64 from 49; Kp 224 from 196 (fp32)


@pytest.mark.parametrize('dt', [FP, BF], ids=key)
@pytest.mark.parametrize('shape', PATCH_CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_stem7_patches_gemm_and_weight_gradient(shape, dt):
    _lib, ops = api()
    lib = _lib.load()
    B, Cin, H, W = shape
    code, p, Cout, K = ops._code(dt), ops._p, 64, Cin * 49
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    M, Kp = B * OH * OW, lib.fva_stem7_kp(code, Cin)
    assert Kp == rr.stem_kp(Cin, dt == BF)
    if dt == FP:
        assert Kp == {3: 160, 1: 64, 4: 224}[Cin]
    g = torch.Generator().manual_seed(H + W + Cin)
    x = torch.randn(shape, generator=g) + 0.25                       # no exact zeros: a zero in P is a border tap or a padding column
    xd = x.to(DEV)

    def launch():
        P = nan_buf((M, Kp), dt)
        _lib.call('fva_stem7_patches', code, p(xd), p(P), B, Cin, H, W, ops._stream())
        return (P.cpu(),)
    P, = twice(launch)
    want = rr.patch_matrix(x, Kp).to(dt)                             # the kernel's one rounding: fp32 -> dtype, to nearest
    assert same_bits(P, want)
    assert not bits(P[:, K:]).any(), 'padding columns are +0'
    taps = rr.patch_matrix(torch.ones(shape), Kp) == 0
    assert not bits(P)[taps].any() and (P[~taps] != 0).all(), 'exactly the border taps and the padding columns are +0'

    # the stem convolution = the 1x1 implicit GEMM over P with the zero-padded filter; its weight gradient = fva_conv_wgrad over P
    w = torch.randn(Cout, Cin, 7, 7, generator=g) * (2.0 / K) ** 0.5
    wpad = torch.zeros(Cout, Kp, 1, 1)
    wpad.view(Cout, Kp)[:, :K] = w.view(Cout, K)
    d = _lib.ConvDesc(code, B, OH, OW, Kp, Cout, 1, 1, 0, 1)
    wf, _ = ops.packed_weights(wpad.to(DEV), d, dt, cache=False)
    Pd = P.to(DEV)
    y = nan_buf((M, Cout), dt)
    _lib.call('fva_conv_fwd', C.byref(d), p(Pd), p(wf), p(y), C.c_void_p(0), ops._stream())
    xs = x.to(dt).double().requires_grad_(False)                     # the operands as stored
    ws = (w.to(dt).double() if dt == BF else w.double()).requires_grad_(True)
    ref = F.conv2d(xs, ws, None, 2, 3)
    e_y = rel_err(y.cpu().view(B, OH, OW, Cout).permute(0, 3, 1, 2), ref)
    dy = torch.randn(B, OH, OW, Cout, generator=g).to(dt)
    ref.backward(dy.double().permute(0, 3, 1, 2))
    dyh = in_halo(dy, 1, 0.0).to(DEV)
    dw = nan_buf((Cout, Kp), FP)
    wsb = lib.fva_conv_wgrad_workspace(C.byref(d))
    ws_buf = torch.empty(max(wsb, 1), dtype=torch.uint8, device=DEV)
    _lib.call('fva_conv_wgrad', C.byref(d), p(Pd), p(dyh), p(dw), 0, p(ws_buf), wsb, ops._stream())
    dw = dw.cpu()
    e_w = rel_err(dw[:, :K].reshape(Cout, Cin, 7, 7), ws.grad)        # the first Cin * 49 columns ARE the OIHW gradient
    assert not dw[:, K:].any(), 'the padding columns of dW are zero (their patches are)'
    print(f'\n  stem7 {key(dt)} {shape}: Kp {Kp}, y {e_y:.2e}, dW {e_w:.2e}')
    assert e_y < TOL[key(dt)] and e_w < TOL[key(dt)]


# ================================================================================================ MaxPool2d(3, 2, 1)
def pool_input(kind, B, H, W, Cc, g):
    x = torch.randn(B, H, W, Cc, generator=g)
    if kind == 'negative':                 # a zero read from the border would win every window
        x = -x.abs() - 0.5
    elif kind == 'relu':                   # more than half exact zeros: ties everywhere
        x = torch.relu(x - 0.3)
    elif kind == 'constant':
        x = torch.full_like(x, 1.25)
    elif kind == 'nan':
        x[0, H // 2, W // 2, 1] = NAN
    return x


@pytest.mark.parametrize('Cc', [64, 24])
@pytest.mark.parametrize('hw', [(8, 8), (7, 5), (2, 2), (1, 1), (16, 6)], ids=lambda s: 'x'.join(map(str, s)))
def test_maxpool3s2_forward_and_backward(hw, Cc):
    _lib, ops = api()
    p = ops._p
    H, W = hw
    B, OH, OW = 2, (H - 1) // 2 + 1, (W - 1) // 2 + 1
    n = 0
    for dt in (BF, FP):
        code = ops._code(dt)
        for kind in ('random', 'negative', 'relu', 'constant', 'nan'):
            for x_pad, o_pad in ((1, 1), (0, 0), (1, 0)):
                g = torch.Generator().manual_seed(H * 100 + W + Cc + x_pad)
                x = pool_input(kind, B, H, W, Cc, g).to(dt)
                if kind == 'relu' and x.numel() >= 1000:
                    assert (x == 0).double().mean() > 0.5
                # the halo border holds ZEROS, as in the model: an all-negative map shows a border read; a second run with NaN borders too
                for fill in (0.0, NAN):
                    xd = in_halo(x, x_pad, fill).to(DEV)

                    def fwd():
                        out = nan_buf((B, OH + 2 * o_pad, OW + 2 * o_pad, Cc), dt)
                        _lib.call('fva_maxpool3s2_fwd', code, p(xd), x_pad, p(out), o_pad, B, H, W, Cc, ops._stream())
                        return (out.cpu(),)
                    out, = twice(fwd)
                    got = interior(out, o_pad, kind, nan_ok=kind == 'nan')
                    want, arg = rr.maxpool3s2(x.double())
                    isn = torch.isnan(want)
                    assert torch.equal(torch.isnan(got), isn) and (isn.any() == (kind == 'nan'))
                    assert same_bits(torch.where(isn, torch.zeros_like(got), got), torch.where(isn, torch.zeros_like(got), want.to(dt))), (kind, key(dt))
                    # backward: dz of small dyadic values, so that the up to four windows that meet in a pixel add exactly in any precision
                    dz = (torch.randint(-31, 32, (B, OH, OW, Cc), generator=g).float() / 8).to(dt)
                    dzd = dz.to(DEV)

                    def bwd():
                        dx = nan_buf((B, H, W, Cc), dt)
                        _lib.call('fva_maxpool3s2_bwd', code, p(dzd), p(xd), x_pad, p(dx), B, H, W, Cc, ops._stream())
                        return (dx.cpu(),)
                    dx, = twice(bwd)
                    ref = rr.maxpool3s2_bwd(dz.double(), x.double())
                    assert not torch.isnan(dx).any()
                    assert torch.equal(dx.double(), ref), (kind, key(dt))                      # the first maximum, overlapping windows summed
                    assert torch.equal(dx.double().sum((1, 2)), dz.double().sum((1, 2)))       # every dz lands on exactly one pixel
                    n += 1
    assert n == 60


# ================================================================================================ the even-pixel subsample
@pytest.mark.parametrize('Cc', [64, 24])
@pytest.mark.parametrize('hw', [(8, 8), (2, 2)], ids=lambda s: 'x'.join(map(str, s)))
def test_subsample2_forward_and_backward(hw, Cc):
    _lib, ops = api()
    p = ops._p
    H, W = hw
    B = 2
    for dt in (BF, FP):
        code = ops._code(dt)
        for x_pad in (0, 1):
            g = torch.Generator().manual_seed(H + Cc + x_pad)
            x = torch.randn(B, H, W, Cc, generator=g).to(dt)
            xd = in_halo(x, x_pad).to(DEV)

            def fwd():
                xs = nan_buf((B, H // 2, W // 2, Cc), dt)
                _lib.call('fva_subsample2_fwd', code, p(xd), x_pad, p(xs), B, H, W, Cc, ops._stream())
                return (xs.cpu(),)
            xs, = twice(fwd)
            assert same_bits(xs, rr.subsample2(x).contiguous())
            gs = (torch.randn(B, H // 2, W // 2, Cc, generator=g) + 3.0).to(dt)                 # no zeros: a zero in dx was written as one
            gd = gs.to(DEV)

            def bwd():
                dx = nan_buf((B, H, W, Cc), dt)                                              # the zeros at odd positions are WRITTEN
                _lib.call('fva_subsample2_bwd', code, p(gd), p(dx), B, H, W, Cc, ops._stream())
                return (dx.cpu(),)
            dx, = twice(bwd)
            assert same_bits(dx, rr.subsample2_bwd(gs))


# ================================================================================================ BatchNorm + add + ReLU
#  B  H   W   C     regime
ADD_RELU_CASES = [
    (2, 4, 4, 64, 'stage-2 width; M = 32 < one reduce block'),
    (1, 3, 5, 2048, 'stage-5 width of the bottlenecks: cpp 256 (bf16) and 512 (fp32: two column passes, beyond the 256 chunks of bn_act.hip)'),
    (3, 8, 8, 256, 'M = 192'),
    (2, 15, 20, 256, 'M = 600: bf16 cpp 32, rpi 8 -> 64 rows per reduce block, 9 full blocks + 24 rows, a lane loops 8 times; fp32 cpp 64, rpi 4 -> 32 rows '
                     'per block, 18 full blocks + 24 rows; 307 200 elements: the rounding bias'),
]
PLACED = 48            # pixels whose first chunk column carries u placed exactly at 0 and one rounding step either side


def step_up(t, up):
    """the neighbour of every element of t (no zeros) in its own format, towards +inf (up) or -inf"""
    if t.dtype == FP:
        return torch.nextafter(t, torch.full_like(t, float('inf') if up else float('-inf')))
    b = bits(t).clone()
    b += torch.where((t > 0) == up, 1, -1).to(torch.int16)
    return b.view(BF)


def add_relu_inputs(dt, B, H, W, Cc, form2, seed):
    g = torch.Generator().manual_seed(seed)
    M = B * H * W
    y = (torch.randn(M, Cc, generator=g) * 1.5 + 0.3).to(dt)
    q = (torch.randn(M, Cc, generator=g) * 1.2 - 0.2).to(dt)
    dz = torch.randn(M, Cc, generator=g).to(dt)
    c = {}
    c['scale'], c['shift'] = signed(g, Cc, 0.3, 2.0), torch.rand(Cc, generator=g) * 2 - 1
    c['mean'], c['rstd'] = torch.randn(Cc, generator=g) * 0.5 + 0.3, torch.rand(Cc, generator=g) + 0.4
    c['gamma'] = signed(g, Cc, 0.5, 1.5)
    c['scale_d'], c['shift_d'] = signed(g, Cc, 0.3, 2.0), torch.rand(Cc, generator=g) * 2 - 1
    c['mean_d'], c['rstd_d'] = torch.randn(Cc, generator=g) * 0.5 - 0.1, torch.rand(Cc, generator=g) + 0.4
    c['gamma_d'] = signed(g, Cc, 0.5, 1.5)
    # u exactly at the kink: in the first 8 channels scale = 1 and shift = 0 (both normalisations), so u = y + q with no rounding at all;
    # q = -y gives u = 0, the neighbours of -y in the tensor's own format give u = +- one rounding step of that format -- exact in fp32
    # and in float64 alike, so the mask is not a matter of precision: 0 and -step are masked, +step is not (where a z stored in bf16
    # and the fp32 u would part ways if the kernel looked at z)
    for k in ('scale', 'scale_d'):
        c[k][:8] = 1.0
    for k in ('shift', 'shift_d'):
        c[k][:8] = 0.0
    placed = torch.zeros(M, Cc, dtype=torch.bool)
    n = min(PLACED, M)
    yy = y[:n, :8]
    yy = torch.where(yy == 0, torch.ones_like(yy), yy)
    y[:n, :8] = yy
    neg = -yy
    rows = torch.arange(n).view(n, 1).expand(n, 8) % 3
    q[:n, :8] = torch.where(rows == 0, neg, torch.where(rows == 1, step_up(neg, True), step_up(neg, False)))
    placed[:n, :8] = True
    return y, q, dz, c, placed


def add_relu_ops(y, q, c, form2):
    """the operand tuple of the restatement's formulas: (y, scale, shift, r, yd, scale_d, shift_d)"""
    return (y, c['scale'], c['shift']) + ((None, q, c['scale_d'], c['shift_d']) if form2 else (q, None, None, None))


#  form2, r_pad (the identity's border; y_d is dense), z_pad = dy_pad
VARIANTS = {'identity-r_pad0': (False, 0, 1), 'identity-r_pad1': (False, 1, 0), 'shortcut': (True, 0, 1)}


@pytest.mark.parametrize('dt', [BF, FP], ids=key)
@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('case', ADD_RELU_CASES, ids=lambda c: 'x'.join(map(str, c[:4])))
def test_bn_add_relu_passes_against_float64(case, variant, dt):
    _lib, ops = api()
    lib = _lib.load()
    B, H, W, Cc, regime = case
    form2, r_pad, pad = VARIANTS[variant]
    M, bf, code, p = B * H * W, dt == BF, ops._code(dt), ops._p
    y, q, dz, c, placed = add_relu_inputs(dt, B, H, W, Cc, form2, 11 + W + Cc + form2)
    o = add_relu_ops(y, q, c, form2)
    u64, main64, R64 = rr.add_relu_u(*o, torch.float64)
    u32, _, _ = rr.add_relu_u(*o, torch.float32)
    umag = torch.maximum(main64.abs(), R64.abs())
    n = min(PLACED, M)
    assert (u64[:n, :8][0::3] == 0).all() and (u64[:n, :8][1::3] > 0).all() and (u64[:n, :8][2::3] < 0).all()
    assert torch.equal(u32[:n, :8].double(), u64[:n, :8]), 'the placed elements are exact in fp32'
    kink = (u64.abs() < sm.limit_of(u64, u32, umag)) & ~placed          # random elements closer to 0 than fp32 resolves: either side is honest
    share = kink.double().mean().item()
    assert share <= KINK_SHARE_MAX, share
    d = {k: v.to(DEV) for k, v in c.items()}
    yd_, dzd = y.to(DEV), dz.to(DEV)
    qd = (q if form2 else in_halo(q.view(B, H, W, Cc), r_pad)).to(DEV)
    none = C.c_void_p(0)
    second = (none, 0, p(qd), p(d['scale_d']), p(d['shift_d'])) if form2 else (p(qd), r_pad, none, none, none)
    second_b = (none, 0, p(qd), p(d['scale_d']), p(d['shift_d']), p(d['mean_d']), p(d['rstd_d'])) if form2 else (p(qd), r_pad, none, none, none, none, none)
    main = (code, p(dzd), p(yd_), p(d['scale']), p(d['shift']), p(d['mean']), p(d['rstd']))

    # ---- forward apply: continuous at the kink, every element is checked
    def apply():
        z = nan_buf((B, H + 2 * pad, W + 2 * pad, Cc), dt)
        _lib.call('fva_bn_add_relu_apply', code, p(yd_), p(d['scale']), p(d['shift']), *second, p(z), pad, B, H, W, Cc, ops._stream())
        return (z.cpu(),)
    z, = twice(apply)
    got = interior(z, pad, regime).reshape(M, Cc)
    z64, mag = rr.add_relu_apply(*o, torch.float64)
    z32, _ = rr.add_relu_apply(*o, torch.float32)
    w_fwd = sm.check(got, z64, z32, mag, bf, bias=bf and got.numel() >= sm.BIAS_MIN_N, what=regime + ' apply')
    assert not bits(got[:n, :8][0::3]).any() and not bits(got[:n, :8][2::3]).any() and (got[:n, :8][1::3] > 0).all()

    # ---- backward pass 1
    nb = lib.fva_bn_add_relu_bwd_blocks(code, M, Cc)
    assert nb > 0
    if Cc == 256 and M == 600:
        assert nb == (10 if bf else 19)
    rows = lib.fva_bn_partial_rows(nb)
    chain = -(-M // nb)
    du64 = rr.add_relu_du(dz, *o)
    assert (du64[:n, :8][0::3] == 0).all() and (du64[:n, :8][2::3] == 0).all() and torch.equal(du64[:n, :8][1::3], dz[:n, :8][1::3].double())

    def reduce():
        part, part_d = nan_buf((rows, 2, Cc), FP), nan_buf((rows, 2, Cc), FP)
        _lib.call('fva_bn_add_relu_bwd_reduce', *main, *second_b, p(part), p(part_d) if form2 else none, nb, B, H, W, Cc, ops._stream())
        return part[:nb].cpu(), part_d[:nb].cpu()
    part, part_d = twice(reduce)
    w_sum = 0.0
    tables = [(part, y, c['mean'], c['rstd'])] + ([(part_d, q, c['mean_d'], c['rstd_d'])] if form2 else [])
    for tab, xop, mean, rstd in tables:
        t64 = rr.add_relu_terms(du64, xop, mean, rstd, torch.float64)
        t32 = rr.add_relu_terms(du64, xop, mean, rstd, torch.float32)
        raw = (dz.double(), dz.double() * (xop.double() - mean.double()) * rstd.double())        # a term's size if its mask flips
        ref = torch.stack([t.sum(0) for t in t64])
        lim = torch.stack([sm.sum_limit(chain, a.abs().sum(0), (b.double() - a).abs().sum(0)) + (r.abs() * kink).sum(0) for a, b, r in zip(t64, t32, raw)])
        sums = tab.double().sum(0)
        assert torch.isfinite(sums).all()
        w_sum = max(w_sum, ((sums - ref).abs() / lim.clamp_min(1e-300)).max().item())
    assert w_sum <= 1.0, f'{regime}: sums worst err / limit {w_sum:.3f}'
    if form2:
        assert torch.equal(part_d[:, 0], part[:, 0]), 'sum dU is shared by both BatchNorms'
    else:
        assert torch.isnan(part_d).all(), 'form 1 writes no second table'

    # ---- fva_bn_bwd_finalize (reused as it is) on the kernel's own tables, then pass 2
    def finalize(tab, gamma, rstd):
        full = torch.zeros((rows, 2, Cc), dtype=FP, device=DEV)
        full[:nb] = tab.to(DEV)
        dgamma, dbeta, coef = nan_buf((Cc,), FP), nan_buf((Cc,), FP), nan_buf((3, Cc), FP)
        _lib.call('fva_bn_bwd_finalize', p(full), nb, rows, M, Cc, p(gamma), p(rstd), p(dgamma), p(dbeta), 0, p(coef), ops._stream())
        sums = tab.double().sum(0)
        fin_lim = (nb + 2) * sm.EPS32 * tab.double().abs().sum(0)
        assert ((dbeta.cpu().double() - sums[0]).abs() <= fin_lim[0]).all() and ((dgamma.cpu().double() - sums[1]).abs() <= fin_lim[1]).all()
        return coef
    coef = finalize(part, d['gamma'], d['rstd'])
    coef_d = finalize(part_d, d['gamma_d'], d['rstd_d']) if form2 else None

    def bwd_apply():
        dy, dy_d, dr = nan_buf((B, H + 2 * pad, W + 2 * pad, Cc), dt), nan_buf((B, H + 2 * pad, W + 2 * pad, Cc), dt), nan_buf((M, Cc), dt)
        _lib.call('fva_bn_add_relu_bwd_apply', *main, p(coef), *second_b, p(coef_d) if form2 else none, p(dy), p(dy_d) if form2 else none, pad,
                  none if form2 else p(dr), B, H, W, Cc, ops._stream())
        return dy.cpu(), dy_d.cpu(), dr.cpu()
    dy, dy_d, dr = twice(bwd_apply)
    keep = ~kink
    w_bwd = 0.0
    outs = [(dy, y, c['mean'], c['rstd'], coef.cpu())] + ([(dy_d, q, c['mean_d'], c['rstd_d'], coef_d.cpu())] if form2 else [])
    for buf, xop, mean, rstd, cf in outs:
        got = interior(buf, pad, regime).reshape(M, Cc)
        r64, mag = rr.add_relu_dy(du64, xop, mean, rstd, cf[0], cf[1], cf[2], torch.float64)
        r32, _ = rr.add_relu_dy(du64, xop, mean, rstd, cf[0], cf[1], cf[2], torch.float32)
        if kink.any():                       # an element on the kink: either side, i.e. with or without its a * dz term
            alt = r64 + cf[0].double() * dz.double() * torch.where(u64 > 0, -1.0, 1.0)
            on = got.double()[kink]
            lo, hi = torch.minimum(r64[kink], alt[kink]), torch.maximum(r64[kink], alt[kink])
            slack = 0.5 * sm.bf16_ulp(hi.abs().maximum(lo.abs())) + 1e-5 * mag[kink]
            assert ((on >= lo - slack) & (on <= hi + slack)).all(), 'an element on the kink is on neither side'
        w_bwd = max(w_bwd, sm.check(got[keep], r64[keep], r32[keep], mag[keep], bf, bias=bf and int(keep.sum()) >= sm.BIAS_MIN_N, what=regime + ' bwd apply'))
    if form2:
        assert torch.isnan(dr).all(), 'form 2 writes no dr'
    else:
        assert torch.isnan(dy_d).all(), 'form 1 writes no dy_d'
        want = du64.to(dt)                   # dr = dU: a selection of dz, bit for bit
        assert same_bits(torch.where(kink, torch.zeros_like(dr), dr), torch.where(kink, torch.zeros_like(dr), want))
        on = dr[kink]
        assert ((on == 0) | (on == dz[kink])).all()
    print(f'\n  bn_add_relu {key(dt)} {variant} [{regime}]: worst err / limit apply {w_fwd:.3f}, sums {w_sum:.3f}, '
          f'bwd apply {w_bwd:.3f}; on the kink (excluded) {int(kink.sum())} of {kink.numel()} = {share:.2e}')
