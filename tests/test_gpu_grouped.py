"""The grouped 3x3 convolution through the C ABI (fva_gconv_fwd / _dgrad / _wgrad), element by element against the float64 grouped
convolution of tests/resnext_restatement.py on exactly the operands uploaded (bf16 operands are rounded once on the host), with the measure
of tests/streaming_measure.py: fp32 outputs (y, dx in fp32 mode, dw in both) within FACTOR x (the error of a plain fp32 torch evaluation +
2^-24 of the element's largest term), bf16 outputs within half a bf16 ulp of the float64 value plus that and unbiased, the statistics table
folded by the real fva_bn_finalize against the float64 mean / variance by sum_limit.  Outputs are allocated full of NaN; the halo is zero
on the ring the padding reads and NaN beyond it (at stride 2 also on the sides of that ring no launch reads); every launch runs twice and must give identical bits.

The kernels' tiles (csrc/grouped.hip), from which the shapes are picked: forward and data gradient -- 256 consecutive output pixels (in
b, y, x order, across rows and images) x a slab of 16 channels, one row of the statistics table per 256 pixels; weight gradient -- 16-pixel
pieces of one output row x a slab of 16 channels, runs of whole output rows (b, oy) per split (more than one row per split only for wide
layers).  So: 10 x 34 at B = 3 (two pieces and two pixels per row, 340 pixels per image: statistics rows straddle both image boundaries),
16 x 17 (a block of 256 pixels plus one row), 16 x 18, 2 x 34 (two pieces plus two pixels), 5 x 7, 2 x 2, and 26 x 2 at C = 1024, B = 3 (three rows per split at stride 1, two at stride 2
with 13 rows per image: splits straddle the images)."""
import ctypes as C

import pytest
import torch

import resnext_restatement as xr
import streaming_measure as sm

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PIX = 256


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _halo(t, pad, dtype, unread=''):
    """t [B, H, W, C] on the host -> device halo buffer: the data, a ring of zeros where the padding is read, NaN beyond it.  ``unread``:
    the sides of that ring no launch of the case may touch, NaN too -- at stride 2 the forward and the weight gradient read source rows
    and columns -1 ... H - 1 only ('br': bottom and right of x), the data gradient output rows and columns 0 ... OH only ('tl' of dy)."""
    B, H, W, Cc = t.shape
    buf = torch.full((B, H + 2 * pad, W + 2 * pad, Cc), float('nan'), dtype=dtype)
    r0, c0 = (pad if 'tl' in unread else pad - 1), (pad if 'tl' in unread else pad - 1)
    r1, c1 = (pad + H if 'br' in unread else pad + H + 1), (pad + W if 'br' in unread else pad + W + 1)
    buf[:, r0:r1, c0:c1] = 0
    buf[:, pad:pad + H, pad:pad + W] = t.to(dtype)
    return buf.to(DEV)


def _nan(shape, dtype):
    return torch.full(shape, float('nan'), dtype=dtype, device=DEV)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _operands(B, H, W, Cc, Cg, stride, bf16, seed):
    g = torch.Generator().manual_seed(seed)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn(B, H, W, Cc, generator=g)
    w = torch.randn(Cc, Cg, 3, 3, generator=g) * (9 * Cg) ** -0.5
    dy = torch.randn(B, OH, OW, Cc, generator=g)
    if bf16:
        x, w, dy = (t.bfloat16().float() for t in (x, w, dy))
    return x, w, dy


def _run(lib_mod, x, w, dy, groups, stride, bf16, in_pad=1, dy_pad=1, stats=True):
    """All three launches, each twice; returns the first results on the host and the finalized statistics."""
    lib = lib_mod.load()
    B, H, W, Cc = x.shape
    Cg = Cc // groups
    OH, OW = dy.shape[1], dy.shape[2]
    dt = torch.bfloat16 if bf16 else torch.float32
    d = lib_mod.GConvDesc(1 if bf16 else 0, B, H, W, Cc, groups, stride, in_pad, dy_pad)
    xb, dyb, wd = _halo(x, in_pad, dt, 'br' if stride == 2 else ''), _halo(dy, dy_pad, dt, 'tl' if stride == 2 else ''), w.to(DEV)
    M = B * OH * OW
    nblk = lib.fva_gconv_stat_blocks(C.byref(d))
    assert nblk == (M + PIX - 1) // PIX
    rows = lib.fva_bn_partial_rows(nblk)
    wsb = lib.fva_gconv_wgrad_workspace(C.byref(d))
    assert wsb > 0
    out = []
    for _ in range(2):
        y, dx, dw = _nan((M, Cc), dt), _nan((B, H, W, Cc), dt), _nan((Cc, Cg, 3, 3), torch.float32)
        tab = _nan((rows, 2, Cc), torch.float32) if stats else None
        ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=DEV)
        lib_mod.call('fva_gconv_fwd', C.byref(d), _p(xb), _p(wd), _p(y), _p(tab), None)
        lib_mod.call('fva_gconv_dgrad', C.byref(d), _p(dyb), _p(wd), _p(dx), None)
        lib_mod.call('fva_gconv_wgrad', C.byref(d), _p(xb), _p(dyb), _p(dw), _p(ws), wsb, None)
        torch.cuda.synchronize()
        out.append((y, dx, dw, tab))
    for a, b in zip(out[0][:3], out[1][:3]):
        assert torch.equal(_bits(a), _bits(b)), 'two launches, two results'
    if stats:
        assert torch.equal(_bits(out[0][3][:nblk]), _bits(out[1][3][:nblk]))
    y, dx, dw, tab = out[0]
    fin = None
    if stats:
        f32 = dict(dtype=torch.float32, device=DEV)
        gamma, beta = torch.ones(Cc, **f32), torch.zeros(Cc, **f32)
        mean, rstd, scale, shift = (torch.empty(Cc, **f32) for _ in range(4))
        lib_mod.call('fva_bn_finalize', _p(tab), nblk, rows, M, Cc, _p(gamma), _p(beta), None, None, None, 0.1, 1e-5, _p(mean), _p(rstd), _p(scale),
                     _p(shift), None)
        torch.cuda.synchronize()
        fin = (mean.cpu().double(), rstd.cpu().double(), nblk)
    return y.cpu().view(B, OH, OW, Cc), dx.cpu(), dw.cpu(), fin


def _compare(x, w, dy, groups, stride, bf16, got, what):
    r64 = xr.gconv_reference(x, w, dy, groups, stride, torch.float64)
    r32 = xr.gconv_reference(x, w, dy, groups, stride, torch.float32)
    y, dx, dw, fin = got
    figs = {}
    for k, g, out_bf16 in (('y', y, bf16), ('dx', dx, bf16), ('dw', dw, False)):
        assert torch.isfinite(g.float()).all(), f'{what}: {k} has elements that were not written, or NaN read from the halo'
        bias = out_bf16 and g.numel() >= sm.BIAS_MIN_N
        figs[k] = sm.check(g.float(), r64[k], r32[k], r64[k + '_mag'], out_bf16, bias=bias, what=f'{what} {k}')
    if fin is not None:
        mean, rstd, nblk = fin
        M = y.numel() // y.shape[-1]
        n = PIX + nblk                                      # the longest chain an fp32 sum over a 256-pixel block and then over the blocks can have
        e1 = (r32['y'].double() - r64['y']).abs().sum((0, 1, 2))
        e2 = ((r32['y'].double() ** 2) - r64['y'] ** 2).abs().sum((0, 1, 2))
        mean64 = r64['s1'] / M
        var64 = r64['s2'] / M - mean64 ** 2
        lim_mean = sm.sum_limit(n, r64['s1_abs'], e1) / M + sm.EPS32 * mean64.abs()
        var_got = 1.0 / rstd ** 2 - 1e-5
        lim_var = sm.sum_limit(n, r64['s2_abs'], e2) / M + 2 * mean64.abs() * lim_mean + lim_mean ** 2 + 4 * sm.EPS32 * (var64 + 1e-5)
        figs['mean'] = ((mean - mean64).abs() / lim_mean).max().item()
        figs['var'] = ((var_got - var64).abs() / lim_var).max().item()
        assert figs['mean'] <= 1.0 and figs['var'] <= 1.0, (what, figs)
    print(f'  {what}: worst err / limit ' + ', '.join(f'{k} {v:.3f}' for k, v in figs.items()))


# (B, H, W, C, Cg, in_pad, dy_pad): what can go wrong, not the workload
SMALL = [(1, 6, 10, Cc, Cg, 1, 1) for Cg in (4, 8, 16, 32, 64) for Cc in (64, 128)]
REAL = [(2, 4, 4, 32 * Cg, Cg, 1, 1) for Cg in (4, 8, 16, 32, 64)]
MAPS = [(3, 10, 34, 128, 4, 1, 1), (3, 10, 34, 64, 64, 1, 1), (1, 16, 18, 64, 8, 1, 1), (2, 2, 34, 64, 16, 1, 1), (1, 2, 2, 128, 32, 1, 1),
        (3, 26, 2, 1024, 32, 1, 1)]
PADS = [(1, 6, 10, 64, 16, 2, 1), (1, 6, 10, 128, 8, 1, 2)]
ODD = [(1, 16, 17, 64, 8, 1, 1), (2, 5, 7, 64, 4, 1, 1)]          # odd maps: stride 1 only (the entry points refuse them at stride 2)
CASES = [(c, s) for c in SMALL + REAL + MAPS + PADS for s in (1, 2)] + [(c, 1) for c in ODD]


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('case,stride', CASES, ids=lambda c: 'x'.join(map(str, c)) if isinstance(c, tuple) else f's{c}')
def test_grouped_convolution_against_float64(case, stride, bf16):
    B, H, W, Cc, Cg, in_pad, dy_pad = case
    lib_mod = _lib()
    x, w, dy = _operands(B, H, W, Cc, Cg, stride, bf16, seed=H * 1000 + W * 10 + Cg + stride)
    got = _run(lib_mod, x, w, dy, Cc // Cg, stride, bf16, in_pad, dy_pad)
    print()
    _compare(x, w, dy, Cc // Cg, stride, bf16, got, f'{case} stride {stride} {"bf16" if bf16 else "f32"}')


def test_eval_mode_forward_takes_no_statistics_table():
    lib_mod = _lib()
    x, w, dy = _operands(1, 6, 10, 64, 8, 1, False, seed=3)
    y, _, _, fin = _run(lib_mod, x, w, dy, 8, 1, False, stats=False)
    assert fin is None
    r64 = xr.gconv_reference(x, w, dy, 8, 1, torch.float64)
    r32 = xr.gconv_reference(x, w, dy, 8, 1, torch.float32)
    sm.check(y, r64['y'], r32['y'], r64['y_mag'], False, what='eval y')


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('c_cg', [(64, 4), (64, 8), (128, 16), (128, 64)])
def test_no_leakage_between_groups(c_cg, stride, bf16):
    """An input that is non-zero in one group only: every output channel outside that group is +0 bit for bit; dy non-zero in another
    group only: dw of every group but that one is +0 bit for bit (and all of dw when x and dy live in different groups)."""
    Cc, Cg = c_cg
    groups = Cc // Cg
    lib_mod = _lib()
    x, w, dy = _operands(2, 6, 10, Cc, Cg, stride, bf16, seed=Cc + Cg)
    g0, g1 = groups // 2, 0
    x0, dy1 = torch.zeros_like(x), torch.zeros_like(dy)
    x0[..., g0 * Cg:(g0 + 1) * Cg] = x[..., g0 * Cg:(g0 + 1) * Cg]
    dy1[..., g1 * Cg:(g1 + 1) * Cg] = dy[..., g1 * Cg:(g1 + 1) * Cg]
    y, dx, dw, _ = _run(lib_mod, x0, w, dy1, groups, stride, bf16)
    inside = torch.zeros(Cc, dtype=torch.bool)
    inside[g0 * Cg:(g0 + 1) * Cg] = True
    assert (_bits(y)[..., ~inside] == 0).all() and (y[..., inside] != 0).any()
    assert (_bits(dw) == 0).all()                                       # x lives in g0, dy in g1: no product belongs to any filter
    in1 = torch.zeros(Cc, dtype=torch.bool)
    in1[g1 * Cg:(g1 + 1) * Cg] = True
    assert (_bits(dx)[..., ~in1] == 0).all() and (dx[..., in1] != 0).any()
    _, _, dw, _ = _run(lib_mod, x, w, dy1, groups, stride, bf16)
    assert (_bits(dw)[~in1] == 0).all() and (dw[in1] != 0).all()
    ref = xr.gconv_reference(x, w, dy1, groups, stride, torch.float64)['dw']
    assert torch.allclose(dw.double(), ref, rtol=1e-5, atol=1e-5)


def test_refusals_return_the_error_code_and_launch_nothing():
    lib_mod = _lib()
    lib = lib_mod.load()
    G = lib_mod.GConvDesc
    f = torch.float32
    xb, dyb, wd = _nan((1, 10, 10, 128), f), _nan((1, 10, 10, 128), f), _nan((128, 4, 3, 3), f)
    y, dx, dw, tab = _nan((64, 128), f), _nan((1, 8, 8, 128), f), _nan((128, 4, 3, 3), f), _nan((4, 2, 128), f)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    for what, d in {'Cg = 3': G(0, 1, 8, 8, 96, 32, 1, 1, 1), 'C = 96': G(0, 1, 8, 8, 96, 24, 1, 1, 1), 'stride 3': G(0, 1, 8, 8, 128, 32, 3, 1, 1),
                    'odd map at stride 2': G(0, 1, 7, 8, 128, 32, 2, 1, 1), 'in_pad 0': G(0, 1, 8, 8, 128, 32, 1, 0, 1)}.items():
        assert lib.fva_gconv_fwd(C.byref(d), _p(xb), _p(wd), _p(y), _p(tab), None) == -1, what
        assert 'fva_gconv_fwd' in lib.fva_last_error().decode()
        assert lib.fva_gconv_dgrad(C.byref(d), _p(dyb), _p(wd), _p(dx), None) == -1, what
        assert lib.fva_gconv_wgrad(C.byref(d), _p(xb), _p(dyb), _p(dw), _p(ws), 1 << 20, None) == -1, what
    ok = G(0, 1, 8, 8, 128, 32, 1, 1, 1)
    assert lib.fva_gconv_wgrad(C.byref(ok), _p(xb), _p(dyb), _p(dw), _p(ws), 16, None) == -3
    torch.cuda.synchronize()
    for t in (y, dx, dw, tab):
        assert torch.isnan(t).all()
    assert not ws.any()
