"""Pins tests/fast_eval_restatement.py (the float64 reference of fva_fast_decode) without a GPU: hand-worked rows, the cases the GPU tests
use leave out zero rows, an fp32 evaluation of the same chain lies inside the derived limits, and two mutants are caught."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fast_eval_restatement as FR  # noqa: E402


def test_hand_worked_rows():
    cls, box, prop, counts, lbs, expected = FR.hand_rows()
    ref = FR.restate(cls, box, prop, counts, len(expected), False, 16.0, (128, 128), 5.0, lbs)
    rows = ref['rows'][0]
    for r, (dropped, cat, what) in enumerate(expected):
        assert bool(ref['drop'][0, r]) == dropped, what
        if dropped:
            assert rows[r].tolist() == [0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0], what
        else:
            assert rows[r, 5:].tolist() == [1.0 if c == cat else 0.0 for c in range(3)], what
    # exp(d2) twice: the decoded box keeps its proposal's aspect ratio although d3 != d2; w = exp(0.2f * 1.5) * 2 * 32
    w, h = rows[0, 2] - rows[0, 0], rows[0, 3] - rows[0, 1]
    assert abs(w / h - 2.0 / 3.0) < 1e-12
    assert abs(w - np.exp(float(np.float32(0.2)) * 1.5) * 64.0) < 1e-9
    assert rows[0, 0] + w / 2 == pytest.approx(320.0, abs=1e-9) and rows[0, 1] + h / 2 == pytest.approx(640.0, abs=1e-9)
    # the ties are ties in float64 too, and the threshold rows sit exactly on / one fp32 step above min_wh
    assert ref['gap'][0, 1] == 0.0 and ref['gap'][0, 2] == 0.0
    up = float(np.nextafter(np.float32(5.0), np.float32(6.0)))
    assert ref['wm'][0, 3] == 0.0 and ref['wm'][0, 4] == up - 5.0 and ref['hm'][0, 5] == 0.0 and ref['hm'][0, 6] == up - 5.0
    # score of the kept rows: the softmax maximum
    p = torch.softmax(cls.double(), dim=1)
    assert rows[0, 4] == pytest.approx(float(p[0, 1]), abs=1e-15) and rows[2, 4] == pytest.approx(float(p[2, 2]), abs=1e-15)


def test_padding_rows_and_multi_reg_column():
    g = torch.Generator().manual_seed(1)
    cls = torch.tensor([[0.0, 1.0, 3.0], [0.0, 3.0, 1.0]])
    box = torch.zeros(2, 12)
    box[0, 8:12] = torch.tensor([1.0, 0.0, 0.0, 0.0])         # row 0's maximum logit is column 2: its deltas are box[8:12]
    box[0, 4:8] = torch.tensor([-5.0, 0.0, 0.0, 0.0])
    box[1, 4:8] = torch.tensor([2.0, 0.0, 0.0, 0.0])
    prop = torch.tensor([[3.0, 3.0, 2.0, 2.0], [3.0, 3.0, 2.0, 2.0]])
    ref = FR.restate(cls, box, prop, [0, 2], 3, True, 16.0, (128, 128))
    assert ref['rows'].shape == (2, 3, 7) and not ref['live'][0].any() and ref['live'][1].tolist() == [True, True, False]
    assert (ref['rows'][0, :, 4] == -1).all() and ref['rows'][1, 2, 4] == -1 and ref['rows'][0, :, :4].abs().sum() == 0
    cx = (ref['rows'][1, :2, 0] + ref['rows'][1, :2, 2]) / 2
    assert cx[0] == pytest.approx((float(np.float32(0.1)) * 2 + 3) * 16) and cx[1] == pytest.approx((float(np.float32(0.1)) * 4 + 3) * 16)
    del g


@pytest.mark.parametrize('name', sorted(FR.CASES))
def test_gpu_cases_leave_out_zero_rows_and_fp32_lies_inside_the_limits(name):
    c = FR.case(name)
    ref = c['ref']
    assert int(FR.undecided(ref).sum()) == 0 and int(FR.undecided(ref, FR.MARGIN_FACTOR).sum()) == 0
    live, kept = ref['live'], ref['live'] & ~ref['drop']
    assert int(live.sum()) == sum(c['counts'])
    if sum(c['counts']) > 10:
        assert int(kept.sum()) >= 5 and int((live & ref['drop'] & (ref['cat'] == 0)).sum()) >= 5          # both outcomes occur
        assert int((live & (ref['cat'] > 0) & ref['drop']).sum()) >= 2                                    # the size filter fires
        assert float(c['cls'].abs().max()) >= 60.0
    # the restatement against itself is clean, and the same rows rounded to fp32 are far inside the limits
    rep = FR.check(ref['rows'].float(), ref, what=name)
    assert rep['kept'] == int(kept.sum())


def _fp32_chain(c):
    """steps 1-9 in fp32 torch on the CPU (torch's exp is within 1 ulp): a stand-in for the kernel"""
    cls, box, prop = c['cls'], c['box'], c['proposals']
    K = cls.size(0)
    m = cls.argmax(1)
    d = (box.view(K, -1, 4)[torch.arange(K), m] if c['multi_reg'] else box) * torch.tensor([0.1, 0.1, 0.2, 0.2])
    x, y = d[:, 0] * prop[:, 2] + prop[:, 0], d[:, 1] * prop[:, 3] + prop[:, 1]
    e = torch.exp(d[:, 2])
    w, h = e * prop[:, 2], e * prop[:, 3]
    score, cat = torch.softmax(cls, dim=1).max(dim=1)
    img = torch.repeat_interleave(torch.arange(len(c['counts'])), torch.tensor(c['counts']))
    lbs = c['letterboxes'] or [(1.0, 0.0, 0.0, float(FR.INPUT_HW[1]), float(FR.INPUT_HW[0]))] * len(c['counts'])
    fr = torch.tensor([list(one) for one in lbs], dtype=torch.float32)[img]
    x = torch.minimum(((x * 16 - fr[:, 1]) / fr[:, 0]).clamp_min(0), fr[:, 3] - 1)
    y = torch.minimum(((y * 16 - fr[:, 2]) / fr[:, 0]).clamp_min(0), fr[:, 4] - 1)
    w = torch.minimum((w * 16 / fr[:, 0]).clamp_min(0), fr[:, 3])
    h = torch.minimum((h * 16 / fr[:, 0]).clamp_min(0), fr[:, 4])
    drop = (cat == 0) | ~((w > 5) & (h > 5))
    rows = torch.zeros(K, 5 + c['C'])
    rows[:, 0] = torch.minimum((x - w / 2).clamp_min(0), fr[:, 3] - 1)
    rows[:, 1] = torch.minimum((y - h / 2).clamp_min(0), fr[:, 4] - 1)
    rows[:, 2] = torch.minimum((x + w / 2).clamp_min(0), fr[:, 3] - 1)
    rows[:, 3] = torch.minimum((y + h / 2).clamp_min(0), fr[:, 4] - 1)
    rows[:, 4] = score
    rows[torch.arange(K), 5 + (cat - 1).clamp_min(0)] = 1.0
    rows[drop] = 0.0
    rows[drop, 4] = -1.0
    out = torch.zeros(len(c['counts']), c['R'], 5 + c['C'])
    out[..., 4] = -1.0
    s = 0
    for b, n in enumerate(c['counts']):
        out[b, :n] = rows[s:s + n]
        s += n
    return out


@pytest.mark.parametrize('name', ['c1_single_input', 'c20_multi_lb', 'c80_multi_lb', 'c80_single_input'])
def test_an_fp32_evaluation_of_the_chain_passes(name):
    c = FR.case(name)
    rep = FR.check(_fp32_chain(c), c['ref'], what=name + ' fp32 chain')
    assert rep['worst_box'] > 0.0                              # it IS a different evaluation, and the limits are not vacuous


@pytest.mark.parametrize('mutant', ['h_uses_d3', 'cat_excludes_bg'])
def test_mutants_are_caught(mutant):
    c = FR.case('c20_multi_lb')
    bad = FR.restate(c['cls'], c['box'], c['proposals'], c['counts'], c['R'], c['multi_reg'], FR.STRIDE, FR.INPUT_HW, 5.0, c['letterboxes'],
                     mutant=mutant)
    rep = FR.compare(bad['rows'].float(), c['ref'])
    assert rep['excused'] == 0
    if mutant == 'h_uses_d3':
        assert rep['worst_box'] > 100.0 or rep['decisions'] > 0
    else:
        assert rep['decisions'] >= 5                            # every background row comes back as a detection
    with pytest.raises(AssertionError):
        FR.check(bad['rows'].float(), c['ref'], what=mutant)


def test_entry_point_refuses_bad_arguments():
    """fva_fast_decode checks its arguments before any launch (no GPU is touched: every call below fails the check)."""
    from fastvision_amd import _lib
    lib = _lib.load()
    assert lib.fva_version() >= 8
    one = C.c_void_p(16)                                        # never dereferenced: the calls fail first
    ok = dict(cls=one, box=one, prop=one, rs=one, K=4, B=1, R=4, C=3, mr=0, stride=16.0, w=128.0, h=128.0, mn=5.0, lb=None, pred=one)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.fva_fast_decode(a['cls'], a['box'], a['prop'], a['rs'], a['K'], a['B'], a['R'], a['C'], a['mr'], a['stride'], a['w'], a['h'],
                                   a['mn'], a['lb'], a['pred'], None)
    for bad in (dict(rs=None), dict(pred=None), dict(cls=None), dict(box=None), dict(prop=None), dict(K=-1), dict(B=0), dict(R=0), dict(C=0),
                dict(mr=2), dict(stride=0.0), dict(w=0.0), dict(h=float('nan')), dict(mn=-1.0), dict(B=40000, R=40000)):
        assert call(**bad) == -1, bad
        assert b'fva_fast_decode' in lib.fva_last_error()
