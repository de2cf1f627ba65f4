"""tests/map_restatement.py pinned without a GPU: the two arg-reductions equal the reference's argsort + two np.unique (the oracle's
CalculateMAP.process_one) on seeded random images, and the demo class's stable sort on exact ties; the C ABI carries fva_map_match and
refuses bad arguments before any pointer is read; process_batch has no CPU path."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import map_restatement as mr
from oracle import detect as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rule_equals_the_reference_matching_on_random_images():
    gen = torch.Generator().manual_seed(20240611)
    est = D.CalculateMAP(mr.THR10)
    want_rows, mismatches, tp50, n_targets = [], 0, 0, set()
    for _ in range(320):
        pred, target = mr.random_image(gen)
        n_targets.add(target.size(0))
        before = len(est.correct_all_images)
        est.process_one(pred, target)
        if pred.size(0) == 0:
            assert len(est.correct_all_images) == before
            continue
        want = est.correct_all_images[-1]
        got = mr.rows_from_rule(pred, target, mr.THR10)
        mismatches += int(not np.array_equal(got, want))
        tp50 += int(want[:, 2].sum())
        want_rows.append(want)
    assert len(want_rows) >= 300 and n_targets == set(range(12))
    assert mismatches == 0
    assert tp50 >= 1000, tp50                         # the comparison is not one of empty matches
    # the cases hold what the rule is about: predictions that lose their target, and flags that differ between thresholds
    allrows = np.concatenate(want_rows)
    assert (allrows[:, 2] > allrows[:, 11]).sum() > 100


def test_rule_equals_the_demo_class_on_exact_ties():
    from fastvision_amd.demos.yolov3_u.utils.map import mean_average_precision
    pred, target = mr.tie_image()
    est = mean_average_precision(mr.THR10)
    est.process_one(pred, target)
    want = est.correct_all_images[0]
    got = mr.rows_from_rule(pred, target, mr.THR10)
    np.testing.assert_array_equal(got, want)
    assert got[:, 2].tolist() == [1.0, 0.0, 1.0]
    # duplicated predictions in the other order of confidence, and the duplicated target listed last: the same outcome by index
    pred2, target2 = pred[[1, 0, 2]], target[[2, 0, 1]]
    est2 = mean_average_precision(mr.THR10)
    est2.process_one(pred2, target2)
    np.testing.assert_array_equal(mr.rows_from_rule(pred2, target2, mr.THR10), est2.correct_all_images[0])
    assert est2.correct_all_images[0][:, 2].tolist() == [1.0, 0.0, 1.0]


def test_pack_batch_and_threshold_boxes_have_their_properties():
    gen = torch.Generator().manual_seed(3)
    images = [mr.random_image(gen) for _ in range(4)]
    dets, kept, targets = mr.pack_batch(images, 40, shuffle=torch.Generator().manual_seed(1), extra_rows=True)
    assert dets.shape == (4, 40, 6) and kept.tolist() == [p.size(0) for p, _ in images]
    assert set(targets[:, 0].tolist()) >= {-1.0, 4.0}
    for b, (pred, target) in enumerate(images):
        assert torch.isnan(dets[b, kept[b]:]).all() and torch.equal(dets[b, :kept[b], 4], pred[:, 1])
        mine = targets[targets[:, 0] == b, 1:]
        assert sorted(mine.tolist()) == sorted(target.tolist())
    from oracle.boxes import cal_iou_batch
    tbox = torch.tensor([[0., 0., 128., 128.]])
    for thr in (0.5, 0.75, 0.95):
        iou = cal_iou_batch(tbox, mr.at_threshold(thr), mode='xyxy').numpy()[0].astype(np.float64)
        assert (np.diff(iou) >= 0).all() and len(set(iou.tolist())) >= 3 and np.diff(iou).max() <= 2.0 ** -22   # an fp32 step or two apart
        above = iou > thr
        assert above.any() and not above.all()                                        # the threshold lies between two of them


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib


def test_map_match_is_declared_bound_and_documented(built):
    lib = built.load()
    assert lib.fva_version() >= 6
    hdr = open(os.path.join(ROOT, 'include', 'fastvision_amd.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert re.search(r'\bfva_map_match\s*\(', hdr)
    assert 'fva_map_match' in built.PROTOTYPES and hasattr(lib, 'fva_map_match')
    assert 'fva_map_match' in doc


def test_map_match_argument_errors_are_reported_before_any_pointer_is_read(built):
    """Every pointer below is 16 or NULL: a call that read one, or launched with it, would crash instead of returning."""
    lib = built.load()
    p = C.c_void_p(16)
    thr = (C.c_double * 16)(*np.linspace(0.5, 0.95, 16))
    ok = dict(det=p, kept=p, B=2, max_det=8, targets=p, T=5, thr=thr, n_thr=10, eps=1e-7, work=p, flags=p)

    def call(**kw):
        a = dict(ok, **kw)
        lib.fva_last_error()
        rc = lib.fva_map_match(a['det'], a['kept'], a['B'], a['max_det'], a['targets'], a['T'], a['thr'], a['n_thr'], a['eps'], a['work'],
                               a['flags'], None)
        return rc, lib.fva_last_error()

    cases = [dict(det=None), dict(kept=None), dict(thr=None), dict(flags=None), dict(targets=None), dict(work=None),
             dict(B=0), dict(B=-1), dict(max_det=0), dict(max_det=-3), dict(T=-1), dict(n_thr=0), dict(n_thr=17), dict(n_thr=-1)]
    for kw in cases:
        rc, msg = call(**kw)
        assert rc != 0 and b'fva_map_match' in msg, (kw, rc, msg)


def test_process_batch_has_no_cpu_path():
    from fastvision_amd.demos.yolov3_u.utils.map import mean_average_precision
    from fastvision_amd.metrics import CalculateMAP
    dets, kept, targets = mr.pack_batch([mr.tie_image()], 8)
    for cls in (CalculateMAP, mean_average_precision):
        est = cls(mr.THR10)
        with pytest.raises(RuntimeError, match='GPU'):
            est.process_batch(dets, kept, targets)
        assert est.correct_all_images == [] and est.seen_all_targets_cls == []
        est.materialize()                                  # nothing pending: nothing happens
        assert est.correct_all_images == []
