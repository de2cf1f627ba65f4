"""The detection-side kernels of csrc/detect.hip at their edges, through the C ABI (fastvision_amd.detect_ops / rpn_ops): decode element by
element against float64 on non-square maps with every accepted level count, anchor count and row length; candidates, rank and NMS exactly,
at the seams of their waves, tiles and blocks, with tied scores, IoUs exactly on the threshold, zero-area boxes and max_nms cuts; the two
matchers exactly, with thresholds that ARE an IoU of the case.  References, inputs and limits: tests/detect_restatement.py (pinned without a
GPU by tests/test_detect_restatement_cpu.py)."""
import contextlib

import numpy as np
import pytest
import torch

import detect_restatement as dr
import streaming_measure as sm

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32 = dr.F64, dr.F32

SCORE = dict(box_mode=1, score_mode=1, rethreshold=0, class_gap=0.0, max_nms=0)     # NMS score = objectness, boxes xyxy: candidate = row


@contextlib.contextmanager
def mask_bytes(limit):
    from fastvision_amd import detect_ops
    old = detect_ops.MASK_BYTES_PER_CALL
    detect_ops.MASK_BYTES_PER_CALL = limit
    try:
        yield
    finally:
        detect_ops.MASK_BYTES_PER_CALL = old


def run_both(p, conf, iou, max_det, mode):
    """rows [n, K] of one image -> the restatement's (detections, source rows), after both branches of nms_batch (all images in one
    fva_nms_select call, and one image at a time) have returned exactly that for the image and for its rows in reverse order"""
    from fastvision_amd import detect_ops
    batch = torch.stack([p, p.flip(0)])
    wants = [dr.nms_restatement(x, conf, iou, max_det, **mode) for x in batch]
    for limit in (detect_ops.MASK_BYTES_PER_CALL, 1):
        with mask_bytes(limit):
            res = detect_ops.nms_batch(batch.to(DEV), conf, iou, max_det, mode)
        for b, ((det, rows), (wd, wr)) in enumerate(zip(res, wants)):
            assert det.shape == wd.shape, (limit, b, det.shape, wd.shape)
            assert torch.equal(rows.cpu(), wr), (limit, b)
            assert torch.equal(det.cpu(), wd), (limit, b)
    return wants[0]


# ---- decode ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['library', 'demo', 'demo_letterbox'])
@pytest.mark.parametrize('name', sorted(dr.DECODE_CASES))
def test_decode_every_element(name, mode):
    from fastvision_amd.detect_ops import yolo_decode
    heads, anchors, strides, lb = dr.decode_case(name)
    variant, box = (0 if mode == 'library' else 1), (lb if mode == 'demo_letterbox' else None)
    r64, mag, e64 = dr.decode_rows(heads, anchors, strides, variant, box, F64)
    r32, _, e32 = dr.decode_rows(heads, anchors, strides, variant, box, F32)
    dev = [h.to(DEV) for h in heads]
    got = yolo_decode(dev, anchors, strides, variant=variant, letterbox=box)
    assert torch.equal(got, yolo_decode([dr.nhwc_view(h) for h in dev], anchors, strides, variant=variant, letterbox=box))
    got = got.cpu()
    if box is not None:
        ex = dr.decode_excused(e64, e32, box[5])
        assert ex.double().mean().item() <= dr.MAX_EXCUSED
        got[..., 4] = torch.where(ex, r64[..., 4].float(), got[..., 4])
        assert torch.equal(got[..., 4] == -1, r64[..., 4] == -1)
    w = sm.check(got, r64, r32, mag, False, factor=sm.FACTOR, what=f'{name} {mode}')
    print(f'decode {name} {mode}: worst err / limit {w:.3f}')


# ---- candidates --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [1, 2, 64, 65, 130])
def test_candidates_at_the_seams_with_class_ties(C):
    """boxes that overlap nothing and max_det = R: the detections ARE the candidates in rank order.  Detections, categories and source rows
    equal the restatement: the lower class wins a tie, objectness == conf_thres is no candidate, rethreshold drops best == conf_thres."""
    from fastvision_amd.detect_ops import nms_batch
    for Rn in (1, 63, 64, 65, 1023, 1024, 1025, 2049):
        pred, info = dr.candidate_case(Rn, C)
        dev = pred.to(DEV)
        for mode in (dict(box_mode=0, score_mode=0, rethreshold=0, class_gap=0.0, max_nms=0),
                     dict(box_mode=0, score_mode=0, rethreshold=1, class_gap=4096.0, max_nms=30000)):
            res = nms_batch(dev, dr.CONF, 0.45, Rn, mode)
            for b in range(3):
                det, rows = res[b]
                wd, wr = dr.nms_restatement(pred[b], dr.CONF, 0.45, Rn, **mode)
                assert torch.equal(rows.cpu(), wr), (Rn, b, mode)
                assert torch.equal(det.cpu(), wd), (Rn, b, mode)
                for bb, r, lo, hi in info['ties']:
                    if bb == b:
                        assert det[rows == r, 5].item() == lo
            assert res[1][0].shape == (0, 6) and res[1][1].numel() == 0


# ---- rank and NMS ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 64, 65, 128, 129, 256, 257, 1100])
def test_rank_order_with_tied_scores(n):
    p, groups = dr.rank_case(n)
    for max_det in sorted({1, 64, n}):
        _, rows = run_both(p, 0.0, 0.45, max_det, SCORE)
        assert rows.numel() == min(max_det, n)
    rows = rows.tolist()
    for grp in groups:
        at = rows.index(grp[0])
        assert rows[at:at + len(grp)] == grp, 'equal scores: the lower candidate index first'


def test_rank_all_scores_equal():
    _, rows = run_both(dr.all_equal_case(300), 0.0, 0.45, 300, SCORE)
    assert rows.tolist() == list(range(300))


@pytest.mark.parametrize('with_gap', [False, True])
@pytest.mark.parametrize('pair', dr.IOU_PAIRS, ids=['iou_0.5', 'iou_0.75'])
def test_iou_exactly_on_the_threshold(pair, with_gap):
    """iou > thr: at iou_thres == IoU both boxes of a pair stay, at the next float below the second goes -- inside a diagonal block of the
    mask and across two blocks, also with class_gap = 4096 added to the coordinates"""
    v, _, _ = pair
    p, idx = dr.pair_case(pair, with_gap)
    mode = dict(SCORE, class_gap=4096.0 if with_gap else 0.0)
    _, at = run_both(p, 0.0, v, p.size(0), mode)
    _, under = run_both(p, 0.0, dr.below(v), p.size(0), mode)
    assert at.numel() == p.size(0)
    assert sorted(set(at.tolist()) - set(under.tolist())) == sorted([idx['b1'], idx['b2']])


def test_zero_area_boxes_and_the_chain():
    p = dr.zero_area_case()
    for thr in (0.0, 0.45):
        _, rows = run_both(p, 0.0, thr, p.size(0), SCORE)
        assert sorted(rows.tolist()) == list(range(p.size(0))), 'a zero-area box is never suppressed and never suppresses'
    p, (ia, ib, ic) = dr.chain_case()
    kept = run_both(p, 0.0, 0.5, p.size(0), SCORE)[1].tolist()
    assert ia in kept and ic in kept and ib not in kept and len(kept) == p.size(0) - 1


@pytest.mark.parametrize('n', [65, 129, 1100])
def test_suppression_across_blocks(n):
    """clustered boxes: bits in every column block of the mask, and as many remv words as n needs"""
    p = dr.clusters_case(n, 60 + n)
    for max_det in (1, 64, n):
        det, rows = run_both(p, 0.0, 0.45, max_det, SCORE)
    assert 8 <= rows.numel() < n


@pytest.mark.parametrize('max_nms', [64, 65, 100])
def test_max_nms_cuts_through_a_tie(max_nms):
    p = dr.max_nms_case()
    for gap in (0.0, 4096.0):
        run_both(p, 0.0, 0.45, p.size(0), dict(SCORE, max_nms=max_nms, class_gap=gap))
    run_both(p, 0.0, 0.45, 10, dict(SCORE, max_nms=max_nms))


# ---- RPN ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('A', [1, 9])
def test_rpn_rows_every_element(A):
    from fastvision_amd.rpn_ops import rpn_proposal_rows
    cls, d, base = dr.rpn_case(3, 5, A)
    got = rpn_proposal_rows(cls.to(DEV), d.to(DEV), base).cpu()
    r64, mag = dr.rpn_rows(cls, d, base, F64)
    r32, _ = dr.rpn_rows(cls, d, base, F32)
    assert torch.all(got[..., 5] == 1)
    w = sm.check(got, r64, r32, mag, False, factor=sm.FACTOR, what=f'rpn rows A={A}')
    print(f'rpn rows 3x5 A={A}: worst err / limit {w:.3f}')


@pytest.mark.parametrize('k', [64, 65])
def test_filter_proposals_with_scores_tied_across_the_cut(k):
    """the rows against float64 with the measure (exp enters); from the device's rows on, the selection (stable: lower row first), the
    suppression and the xywh conversion are exact"""
    from fastvision_amd.rpn_ops import filter_proposals, rpn_proposal_rows
    cls, d, base, tied = dr.rpn_tie_case()
    rows = rpn_proposal_rows(cls.to(DEV), d.to(DEV), base).cpu()
    r64, mag = dr.rpn_rows(cls, d, base, F64)
    r32, _ = dr.rpn_rows(cls, d, base, F32)
    w = sm.check(rows, r64, r32, mag, False, factor=sm.FACTOR, what='rpn tie rows')
    s = rows[0, :, 4]
    assert len(set(s[tied].tolist())) == 1 and int((s > s[tied[0]]).sum()) == 60 and int((s == s[tied[0]]).sum()) == 10
    want, src = dr.proposals_from_rows(rows[0], k, 130, 0.7)
    got = filter_proposals(cls.to(DEV), d.to(DEV), base, k, 130, 0.7)
    assert len(got) == 1 and torch.equal(got[0].cpu(), want)
    few = filter_proposals(cls.to(DEV), d.to(DEV), base, k, 5, 0.7)[0]
    assert torch.equal(few.cpu(), want[:5])
    print(f'rpn tie rows: worst err / limit {w:.3f}; {want.size(0)} proposals of {k}')


# ---- matchers ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 2, 5])
@pytest.mark.parametrize('Na', [1, 255, 256, 257])
def test_matchers_on_their_thresholds(Na, T):
    """rpn_match: best == pos_thr is not positive; fast_match: it is; both: best == neg_thr is not negative; fast_match: best == neg_floor is
    negative (tests/test_detect_restatement_cpu.py shows that the oracle does this on the very anchors).  Identical anchors across a wave
    and across the thread stride: the first claims the box."""
    from fastvision_amd.rpn_ops import fast_match, rpn_match
    from oracle import rpn as R
    anchors, targets, ties = dr.match_case(Na, T)
    thr = {k: dr.f32(v) for k, v in dr.match_thresholds(anchors, targets).items()}
    up = float(np.nextafter(np.float32(thr['floor']), np.float32(1)))
    hi, hi2 = dr.f32(0.999), dr.f32(0.998)
    a_dev, t_dev = anchors.to(DEV), targets.to(DEV)
    for pos, neg in ((dr.f32(0.7), dr.f32(0.3)), (thr['pos'], dr.f32(thr['pos'] / 2)), (hi, thr['neg'])):
        got = rpn_match(a_dev, t_dev, 1, dr.FH, dr.FW, pos, neg).cpu()
        assert torch.equal(got, R.rpn_match(anchors, targets, 1, dr.FH, dr.FW, pos, neg)), (pos, neg)
        for t, i, j in ties:
            assert got[0, i] == t and got[0, j] != t
    ft = dr.fast_targets(targets)
    for pos, neg, floor in ((0.5, 0.5, dr.f32(0.1)), (thr['pos'], dr.f32(thr['pos'] / 2), 0.0), (hi, thr['neg'], 0.0), (hi, hi2, thr['floor']),
                            (hi, hi2, up)):
        got = fast_match(a_dev, ft.to(DEV), 0, pos, neg, floor).cpu()
        assert torch.equal(got, R.fast_match(anchors, ft[:, 2:], pos, neg, floor)), (pos, neg, floor)


def test_matchers_image_whose_boxes_all_belong_to_later_images():
    from fastvision_amd.rpn_ops import fast_match, rpn_match
    from oracle import rpn as R
    anchors, targets, _ = dr.match_case(257, 5)
    targets = targets.clone()
    targets[:, 0] = torch.tensor([1.0, 2.0, 2.0, 1.0, 2.0])
    got = rpn_match(anchors.to(DEV), targets.to(DEV), 3, dr.FH, dr.FW).cpu()
    want = R.rpn_match(anchors, targets, 3, dr.FH, dr.FW)
    assert torch.equal(got, want) and torch.all(got[0] == -2) and (got[1] >= 0).any() and (got[2] >= 0).any()
    ft = dr.fast_targets(targets)
    assert torch.all(fast_match(anchors.to(DEV), ft.to(DEV), 0) == -2)
    for b in (1, 2):
        assert torch.equal(fast_match(anchors.to(DEV), ft.to(DEV), b).cpu(), R.fast_match(anchors, ft[ft[:, 0] == b][:, 2:]))
