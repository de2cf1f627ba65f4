"""The matrix-unit grouped 3x3 convolution through the C ABI (fva_gconv_mfma_pack / _fwd / _dgrad / _wgrad: bf16 tensors, stride 1),
element by element against the float64 grouped convolution of tests/resnext_restatement.py on exactly the operands uploaded, with the
limits of tests/grouped_mfma_measure.py (derived from the number formats; tests/test_grouped_mfma_measure_cpu.py pins them).  The method is
tests/test_gpu_grouped.py's: outputs are allocated full of NaN, every launch runs twice and must give identical bits, and the statistics
table is folded by the real fva_bn_finalize.  In addition both halo tensors are VIEWS into larger allocations full of NaN, so that a staged
read that leaves the tensor and reaches a result shows up.

The kernels' tiles (csrc/grouped_mfma.hip), from which the cases are picked: forward and data gradient -- runs of 256 consecutive PADDED
positions over [B][H + 2][W + 2] x 64 channels, one statistics row per run; weight gradient -- runs of 128 padded positions.  See
grouped_mfma_measure.CASES for what each case stresses."""
import ctypes as C

import pytest
import torch

import grouped_mfma_measure as gm
import resnext_restatement as xr

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 4096                  # NaN elements in front of and behind a halo tensor: more than a row of any case, and 16-byte aligned


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _halo(t):
    """t [B, H, W, C] on the host -> a bf16 halo tensor (border 1, zero) on the device that is a view into the middle of a NaN-filled
    allocation; returns (the allocation, the view)."""
    B, H, W, Cc = t.shape
    n = B * (H + 2) * (W + 2) * Cc
    big = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.bfloat16)
    view = big[GUARD:GUARD + n].view(B, H + 2, W + 2, Cc)
    view.zero_()
    view[:, 1:1 + H, 1:1 + W] = t.bfloat16()
    big = big.to(DEV)
    return big, big[GUARD:GUARD + n].view(B, H + 2, W + 2, Cc)


def _nan(shape, dtype):
    return torch.full(shape, float('nan'), dtype=dtype, device=DEV)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _desc(lib_mod, B, H, W, Cc, groups, dtype=1, stride=1, in_pad=1, dy_pad=1):
    return lib_mod.GConvDesc(dtype, B, H, W, Cc, groups, stride, in_pad, dy_pad)


def _pack(lib_mod, d, w):
    lib = lib_mod.load()
    nb = lib.fva_gconv_mfma_pack_bytes(C.byref(d))
    assert nb > 0 and nb % 1024 == 0
    wd = w.to(DEV)
    out = []
    for _ in range(2):
        wf, wb = _nan((nb // 2,), torch.bfloat16), _nan((nb // 2,), torch.bfloat16)
        lib_mod.call('fva_gconv_mfma_pack', C.byref(d), _p(wd), _p(wf), _p(wb), None)
        torch.cuda.synchronize()
        out.append((wf, wb))
    assert torch.equal(_bits(out[0][0]), _bits(out[1][0])) and torch.equal(_bits(out[0][1]), _bits(out[1][1]))
    return out[0]


def _run(lib_mod, x, w, dy, groups, stats=True):
    """Pack, then all three launches, each twice; returns the first results on the host, the finalized statistics and the tables."""
    lib = lib_mod.load()
    B, H, W, Cc = x.shape
    Cg = Cc // groups
    d = _desc(lib_mod, B, H, W, Cc, groups)
    assert lib.fva_gconv_mfma_serves(C.byref(d)) == 1
    wf, wb = _pack(lib_mod, d, w)
    (xa, xb), (dya, dyb) = _halo(x), _halo(dy)
    M = B * H * W
    nblk = lib.fva_gconv_mfma_stat_blocks(C.byref(d))
    assert nblk == gm.stat_blocks(B, H, W)
    rows = lib.fva_bn_partial_rows(nblk)
    wsb = lib.fva_gconv_mfma_wgrad_workspace(C.byref(d))
    assert wsb > 0
    out = []
    for _ in range(2):
        y, dx, dw = _nan((M, Cc), torch.bfloat16), _nan((B, H, W, Cc), torch.bfloat16), _nan((Cc, Cg, 3, 3), torch.float32)
        tab = _nan((rows, 2, Cc), torch.float32) if stats else None
        ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=DEV)
        lib_mod.call('fva_gconv_mfma_fwd', C.byref(d), _p(xb), _p(wf), _p(y), _p(tab), None)
        lib_mod.call('fva_gconv_mfma_dgrad', C.byref(d), _p(dyb), _p(wb), _p(dx), None)
        lib_mod.call('fva_gconv_mfma_wgrad', C.byref(d), _p(xb), _p(dyb), _p(dw), _p(ws), wsb, None)
        torch.cuda.synchronize()
        out.append((y, dx, dw, tab))
    for a, b in zip(out[0][:3], out[1][:3]):
        assert torch.equal(_bits(a), _bits(b)), 'two launches, two results'
    if stats:
        assert torch.equal(_bits(out[0][3][:nblk]), _bits(out[1][3][:nblk]))
    y, dx, dw, tab = out[0]
    for k, t in (('y', y), ('dx', dx), ('dw', dw)):
        assert torch.isfinite(t.float()).all(), f'{k} has elements that were not written, or NaN read from outside the tensor'
    fin = None
    if stats:
        f32 = dict(dtype=torch.float32, device=DEV)
        gamma, beta = torch.ones(Cc, **f32), torch.zeros(Cc, **f32)
        mean, rstd, scale, shift = (torch.empty(Cc, **f32) for _ in range(4))
        lib_mod.call('fva_bn_finalize', _p(tab), nblk, rows, M, Cc, _p(gamma), _p(beta), None, None, None, 0.1, 1e-5, _p(mean), _p(rstd), _p(scale),
                     _p(shift), None)
        torch.cuda.synchronize()
        fin = (mean.cpu().double(), rstd.cpu().double(), nblk)
    del xa, dya
    return (y.cpu().view(B, H, W, Cc), dx.cpu(), dw.cpu(), fin), (wf.cpu(), wb.cpu())


@pytest.mark.parametrize('case', gm.CASES, ids=gm.case_id)
def test_grouped_mfma_against_float64(case):
    B, H, W, Cc, Cg = case
    lib_mod = _lib()
    x, w, dy = gm.operands(B, H, W, Cc, Cg, seed=H * 1000 + W * 10 + Cg)
    got, (wf, wb) = _run(lib_mod, x, w, dy, Cc // Cg)
    print()
    gm.compare(x, w, dy, Cc // Cg, got, gm.case_id(case))
    # the packed tables, unpacked on the host: the bf16 rounding of w element for element, zeros everywhere else
    for table, dgrad in ((wf, False), (wb, True)):
        back, stray = gm.unpack(table, Cc, Cg, dgrad)
        assert stray == 0 and torch.equal(back, w.bfloat16().float())


def test_pack_rounds_to_nearest_even():
    """Weights that are no bf16 values (the master weight is fp32), ties among them."""
    lib_mod = _lib()
    g = torch.Generator().manual_seed(5)
    w = torch.randn(64, 8, 3, 3, generator=g)
    w.view(-1)[:4] = torch.tensor([1.00390625, 1.01171875, -1.00390625, -1.01171875])      # ties: to even is down, up, and the same negated
    wf, wb = _pack(lib_mod, _desc(lib_mod, 1, 4, 4, 64, 8), w)
    for table, dgrad in ((wf.cpu(), False), (wb.cpu(), True)):
        back, stray = gm.unpack(table, 64, 8, dgrad)
        assert stray == 0 and torch.equal(_bits(back.bfloat16()), _bits(w.bfloat16()))


def test_eval_mode_forward_takes_no_statistics_table():
    lib_mod = _lib()
    x, w, dy = gm.operands(1, 6, 10, 64, 8, seed=3)
    (y, _, _, fin), _ = _run(lib_mod, x, w, dy, 8, stats=False)
    assert fin is None
    ref64, S = gm.references(x, w, dy, 8)
    assert gm.worst(y.float(), ref64['y'], gm.limits(x, 8, ref64, S)['y']) <= 1.0


@pytest.mark.parametrize('c_cg', [(64, 4), (64, 8), (128, 16), (128, 64)])
def test_no_leakage_between_groups(c_cg):
    """An input that is non-zero in one group only: every output channel outside that group is +0 bit for bit; dy non-zero in another
    group only: dw of every group but that one is +0 bit for bit (and all of dw when x and dy live in different groups)."""
    Cc, Cg = c_cg
    groups = Cc // Cg
    lib_mod = _lib()
    x, w, dy = gm.operands(2, 6, 10, Cc, Cg, seed=Cc + Cg)
    g0, g1 = groups // 2, 0
    x0, dy1 = torch.zeros_like(x), torch.zeros_like(dy)
    x0[..., g0 * Cg:(g0 + 1) * Cg] = x[..., g0 * Cg:(g0 + 1) * Cg]
    dy1[..., g1 * Cg:(g1 + 1) * Cg] = dy[..., g1 * Cg:(g1 + 1) * Cg]
    (y, dx, dw, _), _ = _run(lib_mod, x0, w, dy1, groups)
    inside = torch.zeros(Cc, dtype=torch.bool)
    inside[g0 * Cg:(g0 + 1) * Cg] = True
    assert (_bits(y)[..., ~inside] == 0).all() and (y[..., inside] != 0).any()
    assert (_bits(dw) == 0).all()                                       # x lives in g0, dy in g1: no product belongs to any filter
    in1 = torch.zeros(Cc, dtype=torch.bool)
    in1[g1 * Cg:(g1 + 1) * Cg] = True
    assert (_bits(dx)[..., ~in1] == 0).all() and (dx[..., in1] != 0).any()
    (_, _, dw, _), _ = _run(lib_mod, x, w, dy1, groups)
    assert (_bits(dw)[~in1] == 0).all() and (dw[in1] != 0).all()
    ref = xr.gconv_reference(x, w, dy1, groups, 1, torch.float64)['dw']
    assert torch.allclose(dw.double(), ref, rtol=1e-5, atol=1e-5)


REFUSED = {'fp32': dict(dtype=0), 'stride 2': dict(stride=2), 'in_pad 2': dict(in_pad=2), 'dy_pad 2': dict(dy_pad=2)}


def test_refusals_return_the_error_code_and_launch_nothing():
    lib_mod = _lib()
    lib = lib_mod.load()
    bf = torch.bfloat16
    xb, dyb, wd = _nan((1, 12, 12, 128), bf), _nan((1, 12, 12, 128), bf), _nan((128, 4, 3, 3), torch.float32)
    y, dx, dw, tab = _nan((64, 128), bf), _nan((1, 8, 8, 128), bf), _nan((128, 4, 3, 3), torch.float32), _nan((4, 2, 128), torch.float32)
    wf, wb = _nan((1 << 16,), bf), _nan((1 << 16,), bf)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    for what, kw in REFUSED.items():
        d = _desc(lib_mod, 1, 8, 8, 128, 32, **kw)
        assert lib.fva_gconv_mfma_serves(C.byref(d)) == 0, what
        assert lib.fva_gconv_mfma_pack_bytes(C.byref(d)) == 0 and lib.fva_gconv_mfma_stat_blocks(C.byref(d)) == 0, what
        assert lib.fva_gconv_mfma_wgrad_workspace(C.byref(d)) == 0, what
        assert lib.fva_gconv_mfma_pack(C.byref(d), _p(wd), _p(wf), _p(wb), None) == -1, what
        assert 'fva_gconv_mfma_pack' in lib.fva_last_error().decode() and 'stride 1' in lib.fva_last_error().decode()
        assert lib.fva_gconv_mfma_fwd(C.byref(d), _p(xb), _p(wf), _p(y), _p(tab), None) == -1, what
        assert 'fva_gconv_mfma_fwd' in lib.fva_last_error().decode()
        assert lib.fva_gconv_mfma_dgrad(C.byref(d), _p(dyb), _p(wb), _p(dx), None) == -1, what
        assert lib.fva_gconv_mfma_wgrad(C.byref(d), _p(xb), _p(dyb), _p(dw), _p(ws), 1 << 20, None) == -1, what
    ok = _desc(lib_mod, 1, 8, 8, 128, 32)
    assert lib.fva_gconv_mfma_serves(C.byref(ok)) == 1
    assert lib.fva_gconv_mfma_wgrad(C.byref(ok), _p(xb), _p(dyb), _p(dw), _p(ws), 16, None) == -3
    assert 'fva_gconv_mfma_wgrad_workspace' in lib.fva_last_error().decode()
    torch.cuda.synchronize()
    for t in (y, dx, dw, tab, wf, wb):
        assert torch.isnan(t).all()
    assert not ws.any()


def test_serves_is_a_pure_host_answer_and_sets_no_error():
    lib_mod = _lib()
    lib = lib_mod.load()
    bad = _desc(lib_mod, 1, 8, 8, 96, 32)
    assert lib.fva_gconv_fwd(C.byref(bad), None, None, None, None, None) == -1
    before = lib.fva_last_error()
    for d, want in ((_desc(lib_mod, 1, 8, 8, 128, 32, stride=2), 0), (_desc(lib_mod, 2, 56, 56, 128, 32), 1), (_desc(lib_mod, 2, 7, 7, 2048, 32), 1),
                    (_desc(lib_mod, 1, 8, 400, 128, 32), 0), (_desc(lib_mod, 1, 8, 8, 96, 32), 0), (_desc(lib_mod, 1, 8, 8, 128, 2), 1),
                    (_desc(lib_mod, 1, 8, 8, 128, 1), 0)):
        assert lib.fva_gconv_mfma_serves(C.byref(d)) == want
    assert lib.fva_last_error() == before
