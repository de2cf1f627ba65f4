"""Faster R-CNN evaluation on the device: fva_fast_decode against its float64 restatement (tests/fast_eval_restatement.py, limits derived
there), against the present per-image sequence at shared inputs, and the wiring above it -- Fast.detect's one heads pass,
Faster_Rcnn.detect, cfg._fit.Validate / Fit, inference.Inference(batch_size > 1) -- while forward keeps its code path."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fast_eval_restatement as FR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _row_start(counts):
    return torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32).to(DEV)


def _decode(c, prefill=None):
    """rpn_ops.fast_decode, or -- with ``prefill`` -- the entry point itself on an output buffer filled with that value"""
    from fastvision_amd import _lib
    from fastvision_amd.ops import _p, _stream
    from fastvision_amd.rpn_ops import fast_decode
    cls, box, prop = c['cls'].to(DEV), c['box'].to(DEV), c['proposals'].to(DEV)
    rs = _row_start(c['counts'])
    if prefill is None:
        return fast_decode(cls, box, prop, rs, c['R'], FR.STRIDE, FR.INPUT_HW, c['letterboxes'], 5.0, c['multi_reg'])
    B, K = len(c['counts']), cls.size(0)
    pred = torch.full((B, c['R'], 5 + c['C']), prefill, dtype=torch.float32, device=DEV)
    lb = None
    if c['letterboxes'] is not None:
        lb = torch.tensor([list(one) + [5.0] for one in c['letterboxes']], dtype=torch.float32).to(DEV)
    _lib.call('fva_fast_decode', _p(cls), _p(box), _p(prop), _p(rs), K, B, c['R'], c['C'], int(c['multi_reg']), FR.STRIDE,
              float(FR.INPUT_HW[1]), float(FR.INPUT_HW[0]), 5.0, _p(lb) if lb is not None else None, _p(pred), _stream())
    return pred


@pytest.mark.parametrize('name', sorted(FR.CASES))
def test_kernel_vs_restatement(name):
    """C in {1, 20, 80} (81 columns: more than one wave), both heads, both frames, counts (0, 1, 70) in R = 80 rows and K = 1; logits up
    to +-80; the output buffer starts as NaN, so every element the comparison reads was written by the launch."""
    c = FR.case(name)
    got = _decode(c, prefill=float('nan'))
    assert torch.isfinite(got).all()
    FR.check(got, c['ref'], what=name)
    pad = ~c['ref']['live']
    assert (got.cpu()[pad][:, 4] == -1).all() and (got.cpu()[pad][:, :4] == 0).all() and (got.cpu()[pad][:, 5:] == 0).all()
    assert torch.equal(_decode(c), got)                                  # the Python surface is the same launch


def test_hand_built_ties_and_thresholds_are_exact():
    cls, box, prop, counts, lbs, expected = FR.hand_rows()
    c = dict(cls=cls, box=box, proposals=prop, counts=counts, R=len(expected), C=3, multi_reg=False, letterboxes=lbs)
    ref = FR.restate(cls, box, prop, counts, c['R'], False, FR.STRIDE, FR.INPUT_HW, 5.0, lbs)
    got = _decode(c, prefill=float('nan'))
    exact = torch.ones(1, c['R'], dtype=torch.bool)
    rep = FR.compare(got, ref, exact)
    print(rep)
    assert rep['excused'] == 0 and rep['decisions'] == 0 and rep['pattern'] == 0 and rep['worst_box'] <= 1.0 and rep['worst_score'] <= 1.0
    g = got.cpu()[0]
    for r, (dropped, cat, what) in enumerate(expected):
        assert bool(g[r, 4] == -1) == dropped, what
        if not dropped:
            assert g[r, 5:].tolist() == [1.0 if k == cat else 0.0 for k in range(3)], what
    w, h = (g[0, 2] - g[0, 0]).double(), (g[0, 3] - g[0, 1]).double()
    assert abs(w / h - 2.0 / 3.0) < 1e-6                                 # exp(d2) twice


def test_k0_and_argument_checks():
    from fastvision_amd.rpn_ops import fast_decode
    z = torch.zeros(0, 4, device=DEV)
    pred = fast_decode(z, torch.zeros(0, 4, device=DEV), torch.zeros(0, 4, device=DEV), _row_start([0, 0]), 1, 16.0, (64, 96))
    assert tuple(pred.shape) == (2, 1, 8) and (pred[..., 4] == -1).all() and pred[..., :4].abs().sum() == 0 and pred[..., 5:].abs().sum() == 0
    cls, box, prop = torch.zeros(5, 4, device=DEV), torch.zeros(5, 4, device=DEV), torch.ones(5, 4, device=DEV)
    cls[:, 1] = 1.0
    with pytest.raises(ValueError):
        fast_decode(cls, torch.zeros(5, 16, device=DEV), prop, _row_start([5]), 5, 16.0, (64, 96))               # single-reg head, multi-reg box
    with pytest.raises(ValueError):
        fast_decode(cls, box, prop[:4], _row_start([5]), 5, 16.0, (64, 96))
    with pytest.raises(ValueError):
        fast_decode(cls, box, prop, _row_start([5]).long(), 5, 16.0, (64, 96))
    with pytest.raises(ValueError):
        fast_decode(cls, box, prop, _row_start([5]), 5, 16.0, (64, 96), letterboxes=[(1.0, 0, 0, 96, 64)] * 2)
    with pytest.raises(RuntimeError):
        fast_decode(cls.cpu(), box, prop, _row_start([5]), 5, 16.0, (64, 96))
    # a row_start that points past the K rows reads nothing: the rows come back dropped
    pred = fast_decode(cls, box, prop, torch.tensor([3, 9], dtype=torch.int32).to(DEV), 6, 16.0, (64, 96))
    assert (pred[0, :2, 4] > 0).all() and (pred[0, 2:, 4] == -1).all()


# ---- against the present per-image sequence ----------------------------------------------------------------------------------------------
def _present_path(cls, box, xywh, multi_reg, lb, conf, iou):
    """fast.py:103-110 + inference.postProcess + utils.non_max_suppression for ONE image as torch ops on the device, keeping track of the
    source row of every survivor (the present functions drop that index; their results are compared below)."""
    from fastvision_amd.demos.faster_rcnn.models.fast import BOX_STD, Fast
    from fastvision_amd.demos.faster_rcnn.utils import xywh2xyxy
    from fastvision_amd.detect_ops import NMS_DEMO, nms_batch
    rr, pl, pt, ow, oh = lb
    if multi_reg:
        box = Fast._pick_class_box(box, cls.argmax(dim=1))
    box = box * torch.tensor(BOX_STD, device=DEV)
    decoded = torch.stack([box[:, 0] * xywh[:, 2] + xywh[:, 0], box[:, 1] * xywh[:, 3] + xywh[:, 1],
                           torch.exp(box[:, 2]) * xywh[:, 2], torch.exp(box[:, 2]) * xywh[:, 3]], 1)
    scores, categories = torch.softmax(cls, dim=1).max(dim=1)
    keep = categories > 0
    src = torch.nonzero(keep).flatten()
    predict = torch.cat([decoded[keep], (categories[keep, None] - 1).to(decoded), scores[keep, None]], dim=1)
    p = predict.clone()
    p[:, 0:4] = p[:, 0:4] * FR.STRIDE
    p[:, 0] = ((p[:, 0] - pl) / rr).clamp(0, ow - 1)
    p[:, 1] = ((p[:, 1] - pt) / rr).clamp(0, oh - 1)
    p[:, 2] = (p[:, 2] / rr).clamp(0, ow)
    p[:, 3] = (p[:, 3] / rr).clamp(0, oh)
    big = (p[:, 2] > 5) & (p[:, 3] > 5)
    p, src = p[big], src[big]
    p[:, 0:4] = xywh2xyxy(p[:, 0:4])
    p[:, 0], p[:, 2] = p[:, 0].clamp(0, ow - 1), p[:, 2].clamp(0, ow - 1)
    p[:, 1], p[:, 3] = p[:, 1].clamp(0, oh - 1), p[:, 3].clamp(0, oh - 1)
    if p.size(0) == 0:
        return predict, torch.zeros(0, 6, device=DEV), src
    rows = torch.zeros((1, p.size(0), 5 + int(p[:, 4].max().item()) + 1), device=DEV)
    rows[0, :, :4], rows[0, :, 4] = p[:, :4], p[:, 5]
    rows[0, torch.arange(p.size(0), device=DEV), 5 + p[:, 4].long()] = 1.0
    det, idx = nms_batch(rows, conf, iou, 300, NMS_DEMO)[0]
    return predict, det, src[idx]


@pytest.mark.parametrize('name', ['c20_multi_lb', 'c80_single_lb', 'c1_single_lb'])
def test_decode_and_nms_vs_present_path_at_shared_inputs(name):
    from fastvision_amd.demos.faster_rcnn.inference import postProcess
    from fastvision_amd.detect_ops import NMS_DEMO, nms_batch_padded
    c = FR.case(name)
    conf, iou = 0.3, 0.5
    dets, rows, kept = nms_batch_padded(_decode(c), conf, iou, 300, NMS_DEMO)
    kept = kept.cpu().tolist()
    args = types.SimpleNamespace(backbone_stride=FR.STRIDE, inference_conf_thres=conf, inference_iou_thres=iou)
    start, total = 0, 0
    for b, n in enumerate(c['counts']):
        sl = slice(start, start + n)
        start += n
        lb = c['letterboxes'][b]
        if n == 0:
            assert kept[b] == 0
            continue
        predict, det, src = _present_path(c['cls'][sl].to(DEV), c['box'][sl].to(DEV), c['proposals'][sl].to(DEV), c['multi_reg'], lb, conf, iou)
        scores, cats, boxes = postProcess(predict, args, lb[0], lb[1], lb[2], lb[3], lb[4])          # the tracked copy IS the present path
        assert torch.equal(boxes, det[:, :4]) and torch.equal(scores.view(-1), det[:, 4]) and torch.equal(cats.view(-1), det[:, 5])
        assert kept[b] == det.size(0), (b, kept[b], det.size(0))
        if not kept[b]:
            continue
        mine, r = dets[b, :kept[b]].cpu().double(), rows[b, :kept[b]].cpu().long()
        assert torch.equal(r, src.cpu()) and torch.equal(mine[:, 5], det[:, 5].cpu().double())
        lim_box, lim_score = c['ref']['lim_box'][b, r], c['ref']['lim_score'][b, r]
        err_box, err_score = (mine[:, :4] - det[:, :4].cpu().double()).abs(), (mine[:, 4] - det[:, 4].cpu().double()).abs()
        print(name, b, 'kept', kept[b], 'worst box err / limit', float((err_box / lim_box).max()), 'score', float((err_score / lim_score).max()))
        assert (err_box <= lim_box).all() and (err_score <= lim_score).all()
        total += kept[b]
    assert total >= 5


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
NC = 3
BASE_ANCHORS = [[16.0, 16.0], [32.0, 32.0], [24.0, 48.0], [48.0, 24.0]]


@pytest.fixture(scope='module')
def small():
    """a small Faster_Rcnn (3 classes) in eval mode and three 3 x 64 x 96 images: a 4 x 6 feature map"""
    from fastvision_amd.demos.faster_rcnn.models import Faster_Rcnn
    torch.manual_seed(11)
    model = Faster_Rcnn(training=False, num_classes=NC, base_anchors=torch.tensor(BASE_ANCHORS), rpn_post_nms_top_n=40).to(DEV).eval()
    with torch.no_grad():                                   # at random weights background wins every RoI: take it out of the race, and
        model.fast.classifier.weight.mul_(40.0)             # spread the class logits, so that detections exist and clear a low threshold
        model.fast.classifier.weight[0].zero_()
        model.fast.classifier.bias[0] = -100.0
    images = torch.rand(3, 3, 64, 96, generator=torch.Generator().manual_seed(12)).to(DEV)
    return model, images


def _parent_fast_eval(fast, feature_backbone, proposals):
    """the eval branch of Fast.forward as recorded before detect() existed"""
    from fastvision_amd.demos.faster_rcnn.models.fast import BOX_STD, _xyxy
    device = feature_backbone.device
    predicts = []
    std = torch.tensor(BOX_STD, device=device)
    for b in range(feature_backbone.size(0)):
        xywh = proposals[b]
        rois = torch.cat([torch.full((xywh.size(0), 1), float(b), device=device), _xyxy(xywh)], 1)
        cls, box = fast._heads(feature_backbone, rois)
        if fast.fast_multi_reg_head:
            box = fast._pick_class_box(box, cls.argmax(dim=1))
        box = box * std
        decoded = torch.stack([box[:, 0] * xywh[:, 2] + xywh[:, 0], box[:, 1] * xywh[:, 3] + xywh[:, 1],
                               torch.exp(box[:, 2]) * xywh[:, 2], torch.exp(box[:, 2]) * xywh[:, 3]], 1)
        scores, categories = torch.softmax(cls, dim=1).max(dim=1)
        keep = categories > 0
        predicts.append(torch.cat([decoded[keep], (categories[keep, None] - 1).to(decoded), scores[keep, None]], dim=1))
    return predicts


def test_forward_keeps_its_results(small):
    import fastvision_amd
    model, images = small
    with torch.no_grad(), fastvision_amd.compute_dtype(torch.float32):
        feature = model.backbone(images)
        proposals = model.rpn(feature)
        want = _parent_fast_eval(model.fast, feature, proposals)
        got_fast = model.fast(feature, proposals)
        got_model = model(images)
    assert len(got_fast) == len(got_model) == 3
    for w, a, b in zip(want, got_fast, got_model):
        assert w.dim() == 2 and w.size(1) == 6 and torch.equal(w, a) and torch.equal(w, b)
    assert sum(w.size(0) for w in want) > 0


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def test_batched_heads_and_detect(small):
    """ONE heads pass over every image's RoIs gives the per-image logits within the tolerance tests/test_gpu_fc.py holds linear /
    linear_relu to (fp32: 1e-4 of the largest entry); detect returns padded device tensors, and an image without proposals keeps nothing."""
    import fastvision_amd
    from fastvision_amd.demos.faster_rcnn.models.fast import _xyxy
    model, images = small
    with torch.no_grad(), fastvision_amd.compute_dtype(torch.float32):
        feature = model.backbone(images)
        assert tuple(feature.shape[2:]) == (4, 6)
        proposals = model.rpn(feature)
        proposals[1] = proposals[1][:0]
        cls, box, xywh, row_start, R = model.fast._detect_heads(feature, proposals)
        counts = [p.size(0) for p in proposals]
        assert row_start.dtype == torch.int32 and row_start.is_cuda and row_start.cpu().tolist() == [0, counts[0], counts[0], counts[0] + counts[2]]
        assert R == max(counts) and cls.size(0) == sum(counts) and tuple(cls.shape[1:]) == (NC + 1,) and torch.equal(xywh, torch.cat(proposals, 0))
        start = 0
        for b, p in enumerate(proposals):
            rois = torch.cat([torch.full((p.size(0), 1), float(b), device=DEV), _xyxy(p)], 1)
            c1, b1 = model.fast._heads(feature, rois)
            if p.size(0):
                assert _rel(cls[start:start + p.size(0)], c1) < 1e-4 and _rel(box[start:start + p.size(0)], b1) < 1e-4
            start += p.size(0)
        real = model.rpn.filter_proposals

        def without_image_1(*a, **k):
            out = real(*a, **k)
            out[1] = out[1][:0]
            return out
        model.rpn.filter_proposals = without_image_1
        try:
            dets, kept = model.detect(images, 0.05, 0.5, max_det=50)
        finally:
            del model.rpn.filter_proposals
    assert tuple(dets.shape) == (3, 50, 6) and dets.is_cuda and kept.is_cuda and kept.dtype == torch.int32 and tuple(kept.shape) == (3,)
    k = kept.cpu().tolist()
    assert k[1] == 0 and k[0] + k[2] > 0
    for b in (0, 2):
        d = dets[b, :k[b]].cpu()
        assert torch.isfinite(d).all() and (d[:, 4] > 0.05).all() and (d[:, 4, None] <= 1).all() and (d[:, 5] == d[:, 5].round()).all()
        assert d[:, 5].min() >= 0 and d[:, 5].max() <= NC - 1 and (d[:, 4][:-1] >= d[:, 4][1:]).all()
        assert d[:, [0, 2]].min() >= 0 and d[:, [0, 2]].max() <= 95 and d[:, [1, 3]].min() >= 0 and d[:, [1, 3]].max() <= 63
    model.train()
    with pytest.raises(RuntimeError):
        model.detect(images, 0.05, 0.5)
    model.eval()


def _loader(images):
    g = torch.Generator().manual_seed(13)
    batches = []
    for lo, hi in ((0, 2), (1, 3)):
        T = 5
        img = torch.sort(torch.cat([torch.arange(hi - lo), torch.randint(0, hi - lo, (T - (hi - lo),), generator=g)]))[0].float()
        wh = 0.2 + 0.5 * torch.rand(T, 2, generator=g)
        xy = wh / 2 + (1 - wh) * torch.rand(T, 2, generator=g)
        batches.append((images[lo:hi].cpu(), torch.cat([img[:, None], torch.randint(0, NC, (T, 1), generator=g).float(), xy, wh], 1)))
    return batches


def test_validate_equals_per_image_bookkeeping(small):
    """Validate over a two-batch loader = CalculateMAP.process_one fed detect's own detections image by image, with targets converted
    here: the conversion (normalised xywh -> xyxy in input pixels) and the image indexing are under test."""
    import fastvision_amd
    from fastvision_amd.demos.faster_rcnn.cfg._fit import Validate
    from fastvision_amd.metrics import CalculateMAP
    model, images = small
    loader = _loader(images)
    args = types.SimpleNamespace(inference_conf_thres=0.05, inference_iou_thres=0.5)
    thresholds = np.linspace(0.5, 0.95, 10)
    with fastvision_amd.compute_dtype(torch.float32):
        model.train()
        got = Validate(model, loader, args)
        assert model.training
        model.eval()
        got_eval = Validate(model, loader, args, metric=CalculateMAP(thresholds))
        assert not model.training
        ref = CalculateMAP(thresholds)
        seen = 0
        with torch.no_grad():
            for imgs, targets in loader:
                dets, kept = model.detect(imgs.to(DEV), 0.05, 0.5)
                H, W = imgs.shape[2:]
                for b, n in enumerate(kept.cpu().tolist()):
                    t = targets[targets[:, 0] == b]
                    x, y, w, h = t[:, 2], t[:, 3], t[:, 4], t[:, 5]
                    y_true = torch.stack([t[:, 1], (x - w / 2) * W, (y - h / 2) * H, (x + w / 2) * W, (y + h / 2) * H], 1).to(DEV)
                    d = dets[b, :n]
                    ref.process_one(torch.cat([d[:, 5:6], d[:, 4:5], d[:, :4]], 1), y_true)
                    seen += n
    assert seen > 0
    want = ref.fetch()
    for g in (got, got_eval):
        assert np.allclose(g[0], want[0], rtol=0, atol=1e-12) and np.allclose(g[1], want[1], rtol=0, atol=1e-12) and list(g[2]) == list(want[2])
    assert len(want[0]) == 10


def test_fit_validates_after_the_epoch_and_returns_to_training(small, tmp_path, monkeypatch, capsys):
    from fastvision_amd.demos.faster_rcnn.cfg import _fit
    model, images = small
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch, 'save', lambda *a, **k: None)             # the 0.5 GB checkpoint is not what is looked at here
    loader = _loader(images)
    args = types.SimpleNamespace(start_epoch=0, total_epoch=1, inference_conf_thres=0.05, inference_iou_thres=0.5)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    opt = torch.optim.SGD(model.parameters(), lr=1e-6)
    torch.manual_seed(14)
    try:
        _fit.Fit(model, args, opt, loader[:1], validation_loader=loader)
        assert model.training and model.rpn.training and model.fast.training
        out = capsys.readouterr().out
        assert 'mAP@0.5 :' in out and 'mAP@0.5:0.95 :' in out
    finally:
        model.load_state_dict(before)
        model.eval()
        for p in model.parameters():
            p.grad = None


def test_inference_batched_matches_one_by_one(tmp_path, monkeypatch):
    """Inference(batch_size=3) over three PNGs of different shapes against batch_size=1: same keys and result shapes; every detection whose
    score is more than LIM away from the confidence threshold appears in both.  LIM: the heads of the two runs see different row counts
    and agree to 1e-4 of the largest logit (tests/test_gpu_fc.py); a softmax probability moves by at most that much per unit of logit
    change, so with logits of magnitude <= 10 the scores agree to 1e-3; the box deltas (x 0.1 or 0.2, x proposal size <= 8 cells, x
    stride 16 / ratio >= 0.5) move a coordinate by at most 1e-4 * |d| * 51 px: 0.05 px for |d| <= 10."""
    import fastvision_amd
    from PIL import Image
    from fastvision_amd.demos.faster_rcnn import inference
    from fastvision_amd.demos.faster_rcnn.inference import Inference
    real_model_fn = inference.model_fn

    def model_fn(args, base_anchors):                          # as in the ``small`` fixture: background out of the race at random weights
        model = real_model_fn(args=args, base_anchors=base_anchors)
        with torch.no_grad():
            model.fast.classifier.weight.mul_(40.0)
            model.fast.classifier.weight[0].zero_()
            model.fast.classifier.bias[0] = -100.0
        return model
    monkeypatch.setattr(inference, 'model_fn', model_fn)
    rng = np.random.RandomState(3)
    for i, (h, w) in enumerate(((90, 140), (128, 100), (60, 60))):
        Image.fromarray(rng.randint(0, 255, (h, w, 3), dtype=np.uint8)).save(tmp_path / f'im{i}.png')
    conf, LIM, LIM_PX = 0.05, 1e-3, 0.05
    args = types.SimpleNamespace(
        training=False, in_channels=3, num_classes=NC, backbone_stride=16, backbone_output_channels=512, backbone_weights='',
        rpn_positive_iou_thres=0.7, rpn_negative_iou_thres=0.3, rpn_positives_per_image=128, rpn_negatives_per_image=128, rpn_pre_nms_top_n=200,
        rpn_post_nms_top_n=30, rpn_nms_thresh=0.7, fast_multi_reg_head=True, fast_positive_iou_thres=0.5, fast_negative_iou_thres=0.5,
        fast_positives_per_image=16, fast_negatives_per_image=48, fast_roi_pool=7, scales=[16, 32, 64], ratios=[0.5, 1, 2], input_size=128,
        inference_conf_thres=conf, inference_iou_thres=0.5, device=DEV)
    results = []
    with fastvision_amd.compute_dtype(torch.float32):
        for bs in (1, 3):
            torch.manual_seed(15)                                         # model_fn builds the model: the same weights both times
            results.append(Inference(args, str(tmp_path), log=lambda *_: None, batch_size=bs))
    one, three = results
    assert list(one) == list(three) and len(one) == 3
    total = 0
    for f in one:
        for a, b in ((one[f], three[f]), (three[f], one[f])):
            (sa, ca, ba), (sb, cb, bb) = ([t.cpu().double() for t in r] for r in (a, b))
            assert sa.dim() == 2 and sa.size(1) == 1 and ca.shape == sa.shape and tuple(ba.shape) == (sa.size(0), 4)
            for i in torch.nonzero((sa.view(-1) - conf).abs() > LIM).flatten().tolist():
                hit = ((sb.view(-1) - sa[i, 0]).abs() <= LIM) & (cb.view(-1) == ca[i, 0]) & ((bb - ba[i]).abs().max(dim=1).values <= LIM_PX)
                assert hit.any(), (f, i, sa[i], ca[i], ba[i])
                total += 1
    print('detections compared', total)
    assert total > 0
