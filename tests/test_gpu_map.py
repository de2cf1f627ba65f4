"""Validation mAP for a whole batch on the GPU: fva_map_match / CalculateMAP.process_batch give, flag for flag, what process_one gives
on the same device for the same images (the behaviour before the batch path existed); exact IoU ties follow tests/map_restatement.py;
nms_batch_padded is nms_batch without the slicing; process_batch reads nothing back; Fit._val agrees with the oracle loop."""
import os

import numpy as np
import pytest
import torch

import map_restatement as mr

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
DEV = 'cuda:0'


def _per_image(dets, kept, targets):
    """the packed batch as process_one's arguments, image by image (targets in the order a boolean mask leaves them)"""
    for b in range(dets.size(0)):
        d = dets[b, :int(kept[b])]
        yield torch.cat([d[:, 5:6], d[:, 4:5], d[:, 0:4]], dim=1), targets[targets[:, 0] == b, 1:]


def _both(dets, kept, targets, thr=mr.THR10, cls=None):
    """(estimator fed by process_one per image, estimator fed by one process_batch), both materialised"""
    from fastvision_amd.metrics import CalculateMAP
    cls = cls or CalculateMAP
    one, batch = cls(thr), cls(thr)
    for pred, target in _per_image(dets, kept, targets):
        one.process_one(pred.to(DEV), target.to(DEV))
    batch.process_batch(dets.to(DEV), kept.to(DEV), targets.to(DEV))
    batch.materialize()
    return one, batch


def _assert_same(one, batch):
    assert len(batch.correct_all_images) == len(one.correct_all_images)
    for got, want in zip(batch.correct_all_images, one.correct_all_images):
        assert got.dtype == want.dtype == np.float64
        np.testing.assert_array_equal(got, want)
    assert len(batch.seen_all_targets_cls) == len(one.seen_all_targets_cls)
    for got, want in zip(batch.seen_all_targets_cls, one.seen_all_targets_cls):
        np.testing.assert_array_equal(got, want)


def _raw_flags(dets, kept, targets, thr=mr.THR10):
    """fva_map_match itself: flags [B,max_det] as int64"""
    import ctypes as C
    from fastvision_amd import _lib
    from fastvision_amd.ops import _p, _stream
    dets, kept, targets = dets.to(DEV).contiguous(), kept.to(DEV), targets.to(DEV).contiguous()
    thr = np.ascontiguousarray(thr, dtype=np.float64)
    flags = torch.full(dets.shape[:2], -1, dtype=torch.int16, device=DEV)
    work = torch.empty(targets.size(0), dtype=torch.int32, device=DEV)
    _lib.call('fva_map_match', _p(dets), _p(kept), dets.size(0), dets.size(1), _p(targets), targets.size(0),
              thr.ctypes.data_as(C.POINTER(C.c_double)), len(thr), 1e-7, _p(work), _p(flags), _stream())
    return flags.cpu().numpy().view(np.uint16).astype(np.int64)


def test_normal_image_empty_image_and_image_without_targets():
    gen = torch.Generator().manual_seed(11)
    full = mr.random_image(gen, max_targets=6)
    while not (full[0].size(0) and full[1].size(0) >= 3 and full[0].size(0) <= 8):
        full = mr.random_image(gen, max_targets=6)
    no_det = (torch.zeros(0, 6), full[1][:2].clone())
    no_tgt = (full[0][:3].clone(), torch.zeros(0, 5))
    dets, kept, targets = mr.pack_batch([full, no_det, no_tgt], 8)
    assert kept.tolist()[1] == 0 and not (targets[:, 0] == 2).any()
    one, batch = _both(dets, kept, targets)
    assert len(one.correct_all_images) == 2 and len(one.seen_all_targets_cls) == 2      # nothing for kept == 0; seen only with targets
    assert one.correct_all_images[0][:, 2].sum() >= 1 and not one.correct_all_images[1][:, 2:].any()
    _assert_same(one, batch)


def test_loops_cross_the_block_size():
    """kept == max_det == 300 and 300 targets in one image (the kernel's block has 256 threads), a second image beside it"""
    gen = torch.Generator().manual_seed(12)
    cls = torch.randint(0, 3, (300,), generator=gen).float()
    xy = torch.rand(300, 2, generator=gen) * 600
    wh = 20 + torch.rand(300, 2, generator=gen) * 60
    target = torch.cat([cls.view(-1, 1), xy, xy + wh], dim=1)
    perm = torch.randperm(300, generator=gen)
    box = target[perm, 1:] + torch.randn(300, 4, generator=gen) * 3
    pred = torch.cat([target[perm, 0:1], torch.rand(300, 1, generator=gen), box], dim=1)
    dets, kept, targets = mr.pack_batch([(pred, target), mr.random_image(gen)], 300)
    assert kept[0] == 300 and (targets[:, 0] == 0).sum() == 300
    one, batch = _both(dets, kept, targets)
    assert one.correct_all_images[0][256:, 2].sum() > 10 and one.correct_all_images[0][:, 2].sum() > 150
    _assert_same(one, batch)


def test_the_lowest_prediction_keeps_a_target_and_the_loser_gets_nothing():
    # image 0: two predictions on one target, the lower-indexed one with the lower IoU: it wins
    t0 = torch.tensor([[2., 10., 10., 110., 110.]])
    p0 = torch.tensor([[2., 0.3, 10., 10., 110., 90.], [2., 0.9, 10., 10., 110., 108.]])
    # image 1: prediction 1's best target (row 0) is taken by prediction 0 while target row 1 also matches it: it gets nothing
    t1 = torch.tensor([[1., 10., 10., 110., 110.], [1., 10., 30., 110., 130.]])
    p1 = torch.tensor([[1., 0.5, 10., 10., 110., 112.], [1., 0.6, 10., 16., 110., 118.]])
    # image 2: the target with the higher IoU has another class: the prediction takes the one of its own class
    t2 = torch.tensor([[0., 10., 10., 110., 110.], [3., 10., 20., 110., 120.]])
    p2 = torch.tensor([[3., 0.5, 10., 11., 110., 111.]])
    dets, kept, targets = mr.pack_batch([(p0, t0), (p1, t1), (p2, t2)], 8)
    one, batch = _both(dets, kept, targets)
    c = one.correct_all_images
    assert c[0][:, 2].tolist() == [1.0, 0.0] and c[0][0, 2:].sum() < 10                 # the winner's own (lower) IoU sets its flags
    from fastvision_amd.detection.tools import cal_iou_batch
    iou1 = cal_iou_batch(t1[:, 1:].to(DEV), p1[:, 2:].to(DEV), mode='xyxy').cpu()
    assert iou1[0, 1] > iou1[1, 1] > 0.5 and iou1[0, 0] > 0.5                           # the case is what it says
    assert c[1][:, 2].tolist() == [1.0, 0.0]
    iou2 = cal_iou_batch(t2[:, 1:].to(DEV), p2[:, 2:].to(DEV), mode='xyxy').cpu()
    assert iou2[0, 0] > iou2[1, 0] > 0.5 and c[2][0, 2] == 1.0 and c[2][0, 2:].tolist() != [1.0] * 10
    _assert_same(one, batch)


def test_ious_on_the_thresholds():
    """IoUs a step of fp32 around 0.5, 0.75 and 0.95: the kernel's IoU has fva_iou_batch's bits, so its flags equal process_one's"""
    preds, tgts = [], []
    for i, thr in enumerate((0.5, 0.75, 0.95)):
        boxes = mr.at_threshold(thr)
        for j in range(boxes.size(0)):                     # every prediction has a target (and a class) of its own
            c = float(5 * i + j)
            preds.append([c, 0.5, *boxes[j].tolist()])
            tgts.append([c, 0., 0., 128., 128.])
    pred, target = torch.tensor(preds), torch.tensor(tgts)
    dets, kept, targets = mr.pack_batch([(pred, target)], 16)
    one, batch = _both(dets, kept, targets)
    c = one.correct_all_images[0]
    for i, col in enumerate((2, 7, 11)):                   # 0.5, 0.75, 0.95 of linspace(0.5, 0.95, 10)
        grp = c[5 * i:5 * i + 5, col]
        assert grp.min() == 0.0 and grp.max() == 1.0, (i, grp)     # the threshold separates the group
    _assert_same(one, batch)


def test_padded_rows_targets_in_any_order_and_foreign_image_indices():
    gen = torch.Generator().manual_seed(13)
    images = [mr.random_image(gen) for _ in range(5)]
    plain = mr.pack_batch(images, 32, pad=0.0)
    dets, kept, targets = mr.pack_batch(images, 32, pad=float('nan'), shuffle=torch.Generator().manual_seed(2), extra_rows=True)
    assert (targets[:, 0] == -1).any() and (targets[:, 0] == 5).any() and torch.isnan(dets).any()
    one, batch = _both(dets, kept, targets)
    assert sum(c[:, 2].sum() for c in one.correct_all_images) >= 10
    _assert_same(one, batch)
    raw = _raw_flags(dets, kept, targets)
    for b in range(5):
        assert (raw[b, int(kept[b]):] == 0).all()          # written as 0, whatever the rows hold
    # NaN padding instead of zeros, foreign rows and the order of the targets change nothing (no exact ties in these images)
    np.testing.assert_array_equal(raw, _raw_flags(*plain))
    # a NaN box inside the kept rows matches nothing and disturbs no other row
    dets2 = dets.clone()
    victim = int(np.argmax(raw[0, :int(kept[0])] > 0))
    dets2[0, victim, 0] = float('nan')
    raw2 = _raw_flags(dets2, kept, targets)
    assert raw2[0, victim] == 0 and (raw2[1:] == raw[1:]).all()


def test_no_targets_at_all():
    gen = torch.Generator().manual_seed(14)
    images = [(mr.random_image(gen)[0], torch.zeros(0, 5)) for _ in range(3)]
    dets, kept, targets = mr.pack_batch(images, 16)
    assert targets.shape == (0, 6)
    one, batch = _both(dets, kept, targets)
    assert batch.seen_all_targets_cls == [] and len(batch.correct_all_images) == sum(1 for k in kept.tolist() if k)
    _assert_same(one, batch)
    assert (_raw_flags(dets, kept, targets) == 0).all()


@pytest.mark.parametrize('n_thr', [1, 10, 16])
def test_threshold_counts(n_thr):
    gen = torch.Generator().manual_seed(15)
    images = [mr.random_image(gen) for _ in range(4)]
    dets, kept, targets = mr.pack_batch(images, 32)
    thr = np.linspace(0.5, 0.95, n_thr)
    one, batch = _both(dets, kept, targets, thr=thr)
    assert all(c.shape[1] == 2 + n_thr for c in batch.correct_all_images)
    assert sum(c[:, 2].sum() for c in one.correct_all_images) >= 8
    _assert_same(one, batch)
    assert (_raw_flags(dets, kept, targets, thr) < (1 << n_thr)).all()


def test_more_than_sixteen_thresholds_are_refused():
    from fastvision_amd.metrics import CalculateMAP
    dets, kept, targets = mr.pack_batch([mr.tie_image()], 8)
    with pytest.raises(RuntimeError, match='fva_map_match'):
        CalculateMAP(np.linspace(0.5, 0.95, 17)).process_batch(dets.to(DEV), kept.to(DEV), targets.to(DEV))


def test_exact_ties_follow_the_restatement():
    """the library's process_one sorts unstably, so exact ties are compared with the rule (and the demo class, which sorts stably)"""
    from fastvision_amd.demos.yolov3_u.utils.map import mean_average_precision
    from fastvision_amd.detection.tools import cal_iou_batch
    from fastvision_amd.metrics import CalculateMAP
    pred, target = mr.tie_image()
    images = [(pred, target), (pred[[1, 0, 2]], target[[2, 0, 1]])]
    dets, kept, targets = mr.pack_batch(images, 8)
    for cls in (CalculateMAP, mean_average_precision):
        est = cls(mr.THR10)
        est.process_batch(dets.to(DEV), kept.to(DEV), targets.to(DEV))
        est.materialize()
        for (p, t), got in zip(images, est.correct_all_images):
            iou = cal_iou_batch(t[:, 1:].to(DEV), p[:, 2:].to(DEV), mode='xyxy').cpu().numpy()      # the device's own IoU bits
            np.testing.assert_array_equal(got, mr.rows_from_rule(p, t, mr.THR10, iou=iou))
            assert got[:, 2].tolist() == [1.0, 0.0, 1.0]
    demo_one, demo_batch = _both(dets, kept, targets, cls=mean_average_precision)
    _assert_same(demo_one, demo_batch)


def test_fixture_images_in_one_batch():
    from fastvision_amd.metrics import CalculateMAP
    lib = np.load(os.path.join(GOLD, 'eval_lib.npz'))
    n_img, n_correct = lib['e3_n']
    images = [(torch.from_numpy(lib[f'e3_{i}_pred']), torch.from_numpy(lib[f'e3_{i}_target'])) for i in range(n_img)]
    dets, kept, targets = mr.pack_batch(images, 24)
    est = CalculateMAP(np.linspace(0.5, 0.95, 10))
    est.process_batch(dets.to(DEV), kept.to(DEV), targets.to(DEV))
    map_iou, map_cls, idx = est.fetch()                    # fetch() materialises by itself
    assert len(est.correct_all_images) == n_correct
    for i, c in enumerate(est.correct_all_images):
        np.testing.assert_array_equal(c, lib[f'e3_correct{i}'])
    np.testing.assert_allclose(map_iou, lib['e3_map_each_iou'], rtol=1e-12)
    np.testing.assert_allclose(map_cls, lib['e3_map_each_cls'], rtol=1e-12)
    assert idx == lib['e3_cls_idx'].tolist()


@pytest.mark.parametrize('which', ['library', 'demo'])
def test_mixed_calls_keep_the_call_order(which):
    from fastvision_amd.demos.yolov3_u.utils.map import mean_average_precision
    from fastvision_amd.metrics import CalculateMAP
    cls = CalculateMAP if which == 'library' else mean_average_precision
    gen = torch.Generator().manual_seed(16)
    images = [mr.random_image(gen) for _ in range(9)]
    images[4] = (torch.zeros(0, 6), images[4][1])          # an image without detections inside a batch
    only_one, mixed = cls(mr.THR10), cls(mr.THR10)
    for pred, target in images:
        only_one.process_one(pred.to(DEV), target.to(DEV))
    groups = [('one', images[0:1]), ('batch', images[1:4]), ('batch', images[4:6]), ('one', images[6:8]), ('batch', images[8:9])]
    for kind, imgs in groups:
        if kind == 'one':
            for pred, target in imgs:
                mixed.process_one(pred.to(DEV), target.to(DEV))
        else:
            dets, kept, targets = mr.pack_batch(imgs, 40)
            mixed.process_batch(dets.to(DEV), kept.to(DEV), targets.to(DEV))
    want, got = only_one.fetch(), mixed.fetch()
    for a, b in zip(got, want):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    _assert_same(only_one, mixed)


def test_two_runs_give_the_same_bits():
    gen = torch.Generator().manual_seed(17)
    images = [mr.random_image(gen) for _ in range(8)] + [mr.tie_image()]
    dets, kept, targets = mr.pack_batch(images, 64)
    a, b = _raw_flags(dets, kept, targets), _raw_flags(dets, kept, targets)
    assert a.any() and np.array_equal(a, b)


def test_nms_batch_padded_is_nms_batch_without_the_slicing():
    from fastvision_amd.detect_ops import nms_batch, nms_batch_padded, NMS_LIBRARY, NMS_DEMO_BATCH
    from oracle.make_golden import synth_predictions
    preds = torch.stack([synth_predictions(torch.Generator().manual_seed(40 + i), 3000, [4, 0, 9, 2][i], 640) for i in range(4)]).to(DEV)
    for mode in (NMS_LIBRARY, NMS_DEMO_BATCH):
        res = nms_batch(preds, 0.25, 0.45, 50, mode)
        out, rows, kept = nms_batch_padded(preds, 0.25, 0.45, 50, mode)
        assert out.shape == (4, 50, 6) and rows.shape == (4, 50) and kept.shape == (4,) and kept.dtype == torch.int32 and kept.is_cuda
        assert kept.tolist() == [len(r[0]) for r in res] and max(kept.tolist()) > 0
        for b in range(4):
            assert torch.equal(out[b, :int(kept[b])], res[b][0]) and torch.equal(rows[b, :int(kept[b])].long(), res[b][1])
    nothing = nms_batch_padded(preds, 2.0, 0.45, 50, NMS_LIBRARY)                 # no candidate anywhere
    assert nothing[2].tolist() == [0, 0, 0, 0] and nothing[0].shape == (4, 50, 6)
    assert all(len(d) == 0 for d, _ in nms_batch(preds, 2.0, 0.45, 50, NMS_LIBRARY))


def test_process_batch_reads_nothing_back():
    from fastvision_amd.metrics import CalculateMAP
    gen = torch.Generator().manual_seed(18)
    dets, kept, targets = (t.to(DEV) for t in mr.pack_batch([mr.random_image(gen) for _ in range(4)], 32))
    est = CalculateMAP(mr.THR10)
    est.process_batch(dets, kept, targets)                 # the library is loaded and the kernel's code object is on the device
    scratch = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode('error')
        try:
            scratch.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            est.process_batch(dets, kept, targets)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not honoured:
        pytest.skip('this torch build does not raise on a synchronising call under set_sync_debug_mode("error")')
    est.materialize()
    assert len(est.correct_all_images) == 2 * sum(1 for k in kept.tolist() if k)


@pytest.mark.parametrize('shift', [1.5, 0.5])
def test_fit_val_agrees_with_the_oracle_loop(shift):
    """Fit._val on two batches against the same steps through the oracle on the device's decoded rows.  shift: how far the objectness
    bias is pushed down -- 1.5 is test_fit_val_reports_loss_and_map's setting; at 0.5 sigmoid(-0.5) = 0.38 > 0.25 lets rows through."""
    import fastvision_amd
    from fastvision_amd.classfication.models import darknet53
    from fastvision_amd.detection.neck import yolov3neck
    from fastvision_amd.detection.head import yolov3head
    from fastvision_amd.detection.models import yolov3
    from fastvision_amd.loss import Yolov3Loss
    from fastvision_amd.utils import Fit
    from fastvision_amd.synthetic import coco_anchors_px, synthetic_batch
    from oracle import detect as D
    with fastvision_amd.compute_dtype(torch.float32):
        torch.manual_seed(3)
        m = yolov3(backbone=darknet53, neck=yolov3neck, head=yolov3head, anchors=coco_anchors_px(),
                   num_anchors_per_level=[3, 3, 3], in_channels=3, num_classes=80, training=True).to(DEV)
        with torch.no_grad():
            for conv in m.head.heads:
                conv.bias.view(3, 85)[:, 4] -= shift
        crit = Yolov3Loss(m, 0.5, 0.05, 1.0, 0.5)
        images, targets = synthetic_batch(2, 64, seed=9)
        fit = Fit(m, torch.device(DEV), None, None, crit, end_epoch=1, train_loader=[(images, targets)],
                  val_loader=[(images, targets), (images, targets)])
        out = fit._val()
        assert len(out['loss']) == 2 and all(isinstance(l, float) and np.isfinite(l) for l in out['loss'])
        m.eval()
        with torch.no_grad():
            head_out, results = m(images.to(DEV), val=True)
            direct = float(crit(head_out, targets.to(DEV)))
        # the losses read back at the end are the batches' losses (fp32, 2^-24 per rounding: 1e-5 leaves room for sums in another order)
        np.testing.assert_allclose(out['loss'], [direct, direct], rtol=1e-5)
        est = D.CalculateMAP(np.linspace(0.5, 0.95, 10))
        n_det = 0
        for _ in range(2):
            for b in range(2):
                sc, cat, box = D.nms_library(results[b].cpu(), 0.25, 0.45, 300)
                tg = targets[targets[:, 0] == b, 1:].clone()
                tg[:, 1:] = D.xywh2xyxy(tg[:, 1:]) * 64
                est.process_one(torch.cat([cat.float(), sc, box], dim=1), tg)
                n_det += len(sc)
        print(f'shift {shift}: {n_det} detections over the two batches')
        if shift == 0.5:
            assert n_det > 0 and est.correct_all_images        # the comparison below is made
        if not est.correct_all_images:
            assert 'map_each_iou' not in out
            return
        ref_iou, ref_cls, ref_idx = est.fetch()
        np.testing.assert_allclose(out['map_each_iou'], ref_iou, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(out['map_each_cls'], ref_cls, rtol=1e-9, atol=1e-12)
        assert out['map_each_cls_idx'] == ref_idx
