"""The stride-2 matrix-unit grouped 3x3 convolution through the C ABI (fva_gconv_mfma_s2_pack / _fwd / _dgrad / _wgrad), element by element
against resnext_restatement.gconv_reference(..., stride 2, float64) on exactly the operands uploaded.  The method is
tests/test_gpu_grouped_mfma.py's: halo tensors are views into NaN-filled allocations, outputs start full of NaN, every launch runs twice and
must give identical bits, the statistics table is folded by the real fva_bn_finalize.  The limits are those of tests/grouped_mfma_measure.py
with the stride-2 term counts (derived, not observed): y and dx half a bf16 ulp of the reference plus sum_limit(9 Cg, S), dw
sum_limit(B OH OW, S['dw']), statistics gm.stat_limits with RUN = 64, the plane positions per block of the stride-2 forward.

The kernels' tiles (csrc/grouped_mfma.hip): forward -- runs of 64 plane positions over [B][OH + 1][OW + 1]; data gradient -- runs of 128
dy-halo positions over [B][OH + 2][OW + 2]; weight gradient -- runs of 64 plane positions."""
import ctypes as C

import pytest
import torch

import grouped_mfma_measure as gm
import resnext_restatement as xr
import streaming_measure as sm
from test_gpu_grouped_mfma import DEV, _bits, _desc, _halo, _lib, _nan, _p

pytestmark = pytest.mark.gpu

RUN = 64
# (B, H, W, C, Cg): where runs of plane positions can go wrong, not the workload
CASES = [(3, 10, 34, 128, 4), (3, 10, 34, 64, 64),        # runs straddle rows and image boundaries
         (2, 5, 7, 64, 16),                                # odd x odd map
         (2, 7, 14, 64, 8),                                # mixed parity
         (1, 1, 1, 64, 8), (2, 2, 2, 128, 32),             # shifts longer than the map
         (3, 26, 2, 256, 32),                              # two-pixel rows
         (6, 7, 7, 128, 32)                                # several images per run
         ] + [(2, 4, 4, 32 * Cg, Cg) for Cg in (4, 8, 16, 32, 64)]      # the five widths, C = 2048 among them


def _out(n):
    return (n - 1) // 2 + 1


def _operands(B, H, W, Cc, Cg, seed):
    x, w, _ = gm.operands(B, H, W, Cc, Cg, seed)
    return x, w, gm.operands(B, _out(H), _out(W), Cc, Cg, seed + 1)[2]


def _run(lib_mod, x, w, dy, groups, stats=True):
    """Pack, then all three launches, each twice; returns the first results on the host, the finalized statistics and the forward table."""
    lib = lib_mod.load()
    B, H, W, Cc = x.shape
    OH, OW, Cg = _out(H), _out(W), Cc // groups
    d = _desc(lib_mod, B, H, W, Cc, groups, stride=2)
    assert lib.fva_gconv_mfma_s2_serves(C.byref(d)) == 1 and lib.fva_gconv_mfma_serves(C.byref(d)) == 0
    nb = lib.fva_gconv_mfma_s2_pack_bytes(C.byref(d))
    assert nb == lib.fva_gconv_mfma_pack_bytes(C.byref(_desc(lib_mod, B, H, W, Cc, groups)))
    (xa, xb), (dya, dyb), wd = _halo(x), _halo(dy), w.to(DEV)
    M = B * OH * OW
    nblk = lib.fva_gconv_mfma_s2_stat_blocks(C.byref(d))
    assert nblk == (B * (OH + 1) * (OW + 1) + RUN - 1) // RUN
    rows = lib.fva_bn_partial_rows(nblk)
    wsb = lib.fva_gconv_mfma_s2_wgrad_workspace(C.byref(d))
    assert wsb > 0
    out = []
    for _ in range(2):
        wf, wb = _nan((nb // 2,), torch.bfloat16), _nan((nb // 2,), torch.bfloat16)
        y, dx, dw = _nan((M, Cc), torch.bfloat16), _nan((B, H, W, Cc), torch.bfloat16), _nan((Cc, Cg, 3, 3), torch.float32)
        tab = _nan((rows, 2, Cc), torch.float32) if stats else None
        ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=DEV)
        lib_mod.call('fva_gconv_mfma_s2_pack', C.byref(d), _p(wd), _p(wf), _p(wb), None)
        lib_mod.call('fva_gconv_mfma_s2_fwd', C.byref(d), _p(xb), _p(wf), _p(y), _p(tab), None)
        lib_mod.call('fva_gconv_mfma_s2_dgrad', C.byref(d), _p(dyb), _p(wb), _p(dx), None)
        lib_mod.call('fva_gconv_mfma_s2_wgrad', C.byref(d), _p(xb), _p(dyb), _p(dw), _p(ws), wsb, None)
        torch.cuda.synchronize()
        out.append((y, dx, dw, wf, wb, tab))
    for a, b in zip(out[0][:5], out[1][:5]):
        assert torch.equal(_bits(a), _bits(b)), 'two launches, two results'
    if stats:
        assert torch.equal(_bits(out[0][5][:nblk]), _bits(out[1][5][:nblk]))
    y, dx, dw, wf, wb, tab = out[0]
    for k, t in (('y', y), ('dx', dx), ('dw', dw), ('wf', wf), ('wb', wb)):
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
    return (y.cpu().view(B, OH, OW, Cc), dx.cpu(), dw.cpu(), fin), wf.cpu()


def _figures(x, w, dy, groups, got):
    """worst err / limit per output (<= 1 passes)"""
    Cg = x.shape[-1] // groups
    ref64 = xr.gconv_reference(x, w, dy, groups, 2, torch.float64)
    S = xr.gconv_reference(x.abs(), w.abs(), dy.abs(), groups, 2, torch.float64)
    L = sm.sum_limit(9 * Cg, S['y'])
    lim = {'y': 0.5 * sm.bf16_ulp(ref64['y']) + L, 'dx': 0.5 * sm.bf16_ulp(ref64['dx']) + sm.sum_limit(9 * Cg, S['dx']),
           'dw': sm.sum_limit(dy.numel() // dy.shape[-1], S['dw'])}
    y, dx, dw, fin = got
    figs = {}
    for k, g in (('y', y), ('dx', dx), ('dw', dw)):
        assert g.shape == ref64[k].shape, (k, g.shape)
        figs[k] = gm.worst(g.float(), ref64[k], lim[k])
    if fin is not None:
        mean, rstd, nblk = fin
        mean64, var64, lim_mean, lim_var = gm.stat_limits(ref64, L, nblk)
        figs['mean'] = ((mean - mean64).abs() / lim_mean).max().item()
        figs['var'] = ((1.0 / rstd ** 2 - 1e-5 - var64).abs() / lim_var).max().item()
    return figs


@pytest.mark.parametrize('case', CASES, ids=gm.case_id)
def test_grouped_mfma_s2_against_float64(case, monkeypatch):
    B, H, W, Cc, Cg = case
    monkeypatch.setattr(gm, 'RUN', RUN)                     # gm.stat_limits: positions per statistics block
    lib_mod = _lib()
    x, w, dy = _operands(B, H, W, Cc, Cg, seed=H * 1000 + W * 10 + Cg)
    got, wf = _run(lib_mod, x, w, dy, Cc // Cg)
    figs = _figures(x, w, dy, Cc // Cg, got)
    print(f'\n  {gm.case_id(case)}: worst err / limit ' + ', '.join(f'{k} {v:.3f}' for k, v in figs.items()))
    assert all(v <= 1.0 for v in figs.values()), figs
    back, stray = gm.unpack(wf, Cc, Cg, False)              # the forward table has the stride-1 layout
    assert stray == 0 and torch.equal(back, w)


def test_eval_mode_forward_takes_no_statistics_table():
    lib_mod = _lib()
    x, w, dy = _operands(1, 6, 10, 64, 8, seed=3)
    got, _ = _run(lib_mod, x, w, dy, 8, stats=False)
    assert got[3] is None
    assert _figures(x, w, dy, 8, got)['y'] <= 1.0


@pytest.mark.parametrize('c_cg', [(64, 4), (64, 8), (128, 16), (128, 64)])
def test_no_leakage_between_groups(c_cg):
    """x non-zero in one group only: y outside that group is +0 bit for bit; dy non-zero in another group only: the same for dx, and no
    product belongs to any filter."""
    Cc, Cg = c_cg
    groups = Cc // Cg
    x, w, dy = _operands(2, 6, 10, Cc, Cg, seed=Cc + Cg)
    g0, g1 = groups // 2, 0
    x0, dy1 = torch.zeros_like(x), torch.zeros_like(dy)
    x0[..., g0 * Cg:(g0 + 1) * Cg] = x[..., g0 * Cg:(g0 + 1) * Cg]
    dy1[..., g1 * Cg:(g1 + 1) * Cg] = dy[..., g1 * Cg:(g1 + 1) * Cg]
    (y, dx, dw, _), _ = _run(_lib(), x0, w, dy1, groups)
    inside, in1 = torch.zeros(Cc, dtype=torch.bool), torch.zeros(Cc, dtype=torch.bool)
    inside[g0 * Cg:(g0 + 1) * Cg] = True
    in1[g1 * Cg:(g1 + 1) * Cg] = True
    assert (_bits(y)[..., ~inside] == 0).all() and (y[..., inside] != 0).any()
    assert (_bits(dx)[..., ~in1] == 0).all() and (dx[..., in1] != 0).any()
    assert (_bits(dw) == 0).all()


REFUSED = {'fp32': dict(dtype=0), 'stride 1': dict(stride=1), 'in_pad 2': dict(in_pad=2), 'dy_pad 2': dict(dy_pad=2), 'C 96': dict(Cc=96, groups=24),
           'Cg 2': dict(groups=64), 'too wide': dict(W=400)}


@pytest.mark.parametrize('what', list(REFUSED))
def test_refusals_return_the_error_code_and_launch_nothing(what):
    lib_mod = _lib()
    lib = lib_mod.load()
    bf = torch.bfloat16
    kw = dict(dict(B=1, H=8, W=8, Cc=128, groups=32, stride=2), **REFUSED[what])
    d = _desc(lib_mod, **kw)
    xb, dyb, wd = _nan((1, 10, 402, 128), bf), _nan((1, 10, 402, 128), bf), _nan((128, 4, 3, 3), torch.float32)
    y, dx, dw, tab = _nan((8 * 400, 128), bf), _nan((1, 8, 400, 128), bf), _nan((128, 4, 3, 3), torch.float32), _nan((64, 2, 128), torch.float32)
    wf, wb = _nan((1 << 16,), bf), _nan((1 << 16,), bf)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    assert lib.fva_gconv_mfma_s2_serves(C.byref(d)) == 0
    assert lib.fva_gconv_mfma_s2_pack_bytes(C.byref(d)) == 0 and lib.fva_gconv_mfma_s2_stat_blocks(C.byref(d)) == 0
    assert lib.fva_gconv_mfma_s2_wgrad_workspace(C.byref(d)) == 0
    for name, args in (('pack', (_p(wd), _p(wf), _p(wb), None)), ('fwd', (_p(xb), _p(wf), _p(y), _p(tab), None)),
                       ('dgrad', (_p(dyb), _p(wb), _p(dx), None)), ('wgrad', (_p(xb), _p(dyb), _p(dw), _p(ws), 1 << 20, None))):
        assert getattr(lib, 'fva_gconv_mfma_s2_' + name)(C.byref(d), *args) == -1, name
        msg = lib.fva_last_error().decode()
        assert 'fva_gconv_mfma_s2_' + name in msg and 'stride 2' in msg
    torch.cuda.synchronize()
    for t in (y, dx, dw, tab, wf, wb):
        assert torch.isnan(t).all()
    assert not ws.any()
