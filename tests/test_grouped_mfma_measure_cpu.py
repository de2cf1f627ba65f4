"""tests/grouped_mfma_measure.py pinned without a GPU: a plain fp32 evaluation of the restatement, stored as bf16, passes the limits at
every case of the GPU suite, and the same evaluation with one filter tap dropped fails them by two orders of magnitude -- so the limits
are neither out of an honest kernel's reach nor loose enough to miss a lost tap.  The packed-table reader is pinned on a table built here
from the layout in include/fastvision_amd.h."""
import pytest
import torch

import grouped_mfma_measure as gm
import resnext_restatement as xr


def _evaluate(x, w, dy, groups, dt=torch.float32):
    """What a kernel would hand back: y and dx as bf16, dw as fp32, the statistics folded in float64 from the fp32 sums."""
    r = xr.gconv_reference(x, w, dy, groups, 1, dt)
    B, H, W, _ = x.shape
    M = B * H * W
    mean = r['s1'].double() / M
    var = r['s2'].double() / M - mean ** 2
    fin = (mean, 1.0 / torch.sqrt(var + 1e-5), gm.stat_blocks(B, H, W))
    return r['y'].bfloat16(), r['dx'].bfloat16(), r['dw'].float(), fin


@pytest.fixture(scope='module', params=gm.CASES, ids=gm.case_id)
def case(request):
    B, H, W, Cc, Cg = request.param
    x, w, dy = gm.operands(B, H, W, Cc, Cg, seed=H * 1000 + W * 10 + Cg)
    return x, w, dy, Cc // Cg, gm.case_id(request.param)


def test_a_plain_fp32_evaluation_passes(case):
    x, w, dy, groups, what = case
    print()
    figs = gm.compare(x, w, dy, groups, _evaluate(x, w, dy, groups), what)
    assert set(figs) == {'y', 'dx', 'dw', 'mean', 'var'}


def test_a_dropped_tap_fails_by_two_orders_of_magnitude(case):
    x, w, dy, groups, what = case
    ref64, S = gm.references(x, w, dy, groups)
    lim = gm.limits(x, groups, ref64, S)
    w_less = w.clone()
    w_less[:, :, 1, 2] = 0                                     # a tap every map has pixels for, the 2 x 2 one included
    y, dx, dw, fin = _evaluate(x, w_less, dy, groups)
    dw = xr.gconv_reference(x, w, dy, groups, 1, torch.float32)['dw'].clone()
    dw[:, :, 1, 2] = 0                                         # the weight gradient loses the tap's own elements
    print()
    for k, g in (('y', y), ('dx', dx), ('dw', dw)):
        ratio = gm.worst(g.float(), ref64[k], lim[k])
        print(f'  {what} {k}: one tap dropped, worst err / limit {ratio:.1f}')
        assert ratio >= 100.0, (what, k, ratio)
    with pytest.raises(AssertionError):
        gm.compare(x, w, dy, groups, (y, dx, dw, fin), what)


@pytest.mark.parametrize('Cg', [4, 8, 16, 32, 64])
@pytest.mark.parametrize('dgrad', [False, True], ids=['fwd', 'dgrad'])
def test_unpack_reads_the_documented_layout(Cg, dgrad):
    """A table filled element by element from the header's formulas (scalar code, no index arithmetic shared with unpack)."""
    Cc = 64 if Cg < 64 else 128
    w = torch.arange(Cc * Cg * 9, dtype=torch.float32).view(Cc, Cg, 3, 3) % 251 + 1
    steps = 9 * (Cg // 32) if Cg >= 32 else 5
    table = torch.zeros(Cc // 16, steps, 64, 8)
    wf = w.view(Cc, Cg, 9)
    for slab in range(Cc // 16):
        for step in range(steps):
            for lane in range(64):
                for j in range(8):
                    m, k = lane % 16, 8 * (lane // 16) + j
                    c = 16 * slab + m
                    if Cg >= 32:
                        tap, kc, gb = step // (Cg // 32), 32 * (step % (Cg // 32)) + k, (c // Cg) * Cg
                        v = wf[gb + kc, c - gb, 8 - tap] if dgrad else wf[c, kc, tap]
                    else:
                        tap, kc = 2 * step + k // 16, k % 16
                        if tap > 8 or kc // Cg != m // Cg:
                            continue
                        v = wf[16 * slab + kc, m % Cg, 8 - tap] if dgrad else wf[c, kc % Cg, tap]
                    table[slab, step, lane, j] = v
    got, stray = gm.unpack(table.bfloat16(), Cc, Cg, dgrad)
    assert stray == 0 and torch.equal(got, w.bfloat16().float())
    if Cg < 32:
        table[0, 4, 32, 0] = 1                                 # step 4, k = 16: the tenth half-step, which must stay zero
        assert gm.unpack(table.bfloat16(), Cc, Cg, dgrad)[1] == 1
